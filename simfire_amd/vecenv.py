"""``BatchedFireEnv``: a small Gym-style vector environment on top of ``BatchedFireSimulation``.

``step(actions)`` is one ``sf_agents_step`` - moves, control lines, the fire update, reward, done, episode statistics and the reset
of finished environments, all on the device - followed by one ``observe``.  Every return is a torch CUDA tensor; nothing is read
back to the host.  The simulation's handle works on a stream of its own that torch does not know, and ``BatchedFireSimulation``
keeps it in async mode, so ``reset`` and ``step`` wait for that stream once (``engine.sync()``) before they return: the tensors
are complete when the caller's torch code reads them.
"""
import numpy as np

# action word = move + 5 * interact
MOVES = ("stay", "up", "down", "left", "right")                  # row - 1, row + 1, column - 1, column + 1
INTERACTIONS = ("none", "fireline", "scratchline", "wetline")
N_ACTIONS = len(MOVES) * len(INTERACTIONS)


def action_word(move, interact=0):
    """The int32 action word of (move, interact), each an index or a name of ``MOVES`` / ``INTERACTIONS``."""
    m = MOVES.index(move) if isinstance(move, str) else int(move)
    i = INTERACTIONS.index(interact) if isinstance(interact, str) else int(interact)
    if not (0 <= m < len(MOVES) and 0 <= i < len(INTERACTIONS)):
        raise ValueError(f"action_word: move {move!r}, interact {interact!r}")
    return m + 5 * i


class BatchedFireEnv:
    """``sim.n_envs`` environments with ``n_agents`` agents each.

    ``start_xy``: int [n_agents, 2] (the same start cells in every environment) or [n_envs, n_agents, 2], (column, row).
    ``weights``: the reward is ``w0 * newly burning or burned cells + w1 * points drawn + w2 * agents standing in the fire +
    w3 * moves that would have left the grid``.  ``only_unburned``: lines are drawn on UNBURNED cells only.  An episode ends when
    the fire is out (or the simulation QUIT), with ``done_on_burn`` when an agent stands in the fire, with ``max_ticks > 0`` after
    that many ticks; with ``auto_reset`` a finished environment is re-ignited at ``sim.ignitions[e]`` (as they stand when the
    environment is built) inside the same ``step``, its agents go back to their start cells, and the observation returned is the new
    episode's - or, after ``sim.randomize_episodes``, at a drawn cell, under a drawn wind, with drawn start cells (DESIGN.md
    section 19).  ``obs``: keyword arguments of ``BatchedFireSimulation.observe`` (``channels`` first of all); its ``agents`` are
    the device positions.

    ``values``: a value plane (``BatchedFireSimulation.set_values``); ``info["value_lost"]`` is then the int64 tensor of what the
    tick's fire reached, a view of the device buffer the next ``step`` overwrites.  ``value_weight``: the reward gets the fifth term
    ``value_weight * value_lost``.  Both default to off: calls and outputs are what they are without them.

    ``fire_distance``: ``None``, or a dict with ``status`` (BurnStatus members, names or ints; default BURNING) and ``max_dist`` (an
    integer number of cells, default no cap): ``info["fire_distance"]`` is then float32 [n_envs, n_agents], the distance in cells from
    every agent to the nearest selected cell (``FireEngine.distance``), taken from the state the observation
    shows - after a tick that re-ignited an environment, the new episode's.  Off by default: calls and ``info`` are what they are
    without it.

    ``reach``: ``None``, or a dict with ``source``, ``through`` (BurnStatus members, names or ints; default BURNING / UNBURNED),
    ``connectivity`` (4, 8 or None: the simulation's ``diagonal_spread``) and ``value`` (bool): ``info["reach_cells"]`` is then int32
    [n_envs], the number of cells the fire can still get to (``FireEngine.reach``), ``info["agent_exposed"]``
    int32 [n_envs, n_agents], 1 where an agent stands in that set, and with ``value`` ``info["reach_value"]`` int64 [n_envs], the value
    plane summed over it - all from the state the observation shows.  Off by default: calls and ``info`` are what they are without it.

    ``moves_to``: ``None``, or a dict with ``target``, ``through`` (BurnStatus members, names or ints; default BURNING / UNBURNED),
    ``passable``, ``targets`` (uint8 CUDA [H, W] or [n_envs, H, W]) and ``max_moves``: ``info["moves_to"]`` is then int32
    [n_envs, n_agents], the number of moves every agent needs to step onto a target cell through walkable cells
    (``FireEngine.walk``), and ``info["move_toward"]`` int32 [n_envs, n_agents] the first move of a shortest
    route as a move code 1..4 (0: stay) - an action word with ``interact = 0`` that can be fed straight back to ``step`` -, both from
    the state the observation shows.  Agents are not routed around each other.  Off by default: calls and ``info`` are what they are
    without it.

    ``behavior``: ``None``, or a dict with ``summary`` (BurnStatus members, names or ints; default BURNING), ``edges`` and
    ``flame_limit`` (checked, but a tick writes no plane): ``info["flame_length"]`` is then float32 [n_envs, n_agents], the largest flame length (ft)
    among the ``summary`` cells of the 3 x 3 block around every agent (0: none), and ``info["max_flame"]`` float32 [n_envs] the
    largest over the environment (``FireEngine.behavior``), both from the state the observation shows.  Off by
    default: calls and ``info`` are what they are without it.

    ``time_to_fire``: ``None``, or a dict with ``source``, ``through`` (BurnStatus members, names or ints; default BURNING /
    UNBURNED), ``passable`` (uint8 CUDA [H, W] or [n_envs, H, W]) and ``max_minutes``: ``info["minutes_to_fire"]`` is then float32
    [n_envs, n_agents], the minimum travel time of the fire to every agent's cell in minutes (``FireEngine.travel``, the point form;
    DESIGN.md section 26) - on a cell the fire cannot enter, such as the line an agent has just drawn, the time at which it would be
    reached were it passable -, from the state the observation shows.  A forecast over the rates of spread, not the automaton's own
    arrival.  Off by default: calls and ``info`` are what they are without it.

    ``perimeter``: ``None``, or a dict with ``status`` (BurnStatus members, names or ints; default BURNING | BURNED):
    ``info["fire_perimeter"]`` is then int32 [n_envs], the length of the fire's edge in cell edges, and ``info["fire_cells"]`` int32
    [n_envs] the cells of the set (``FireEngine.perimeter``, the summary form: one streaming launch, nothing is traced or read back;
    DESIGN.md section 27), both from the state the observation shows.  Off by default: calls and ``info`` are what they are
    without it.

    ``escape``: ``None``, or a dict with ``horizon_minutes`` and any of ``target``, ``targets``, ``through``, ``passable``,
    ``minutes_per_move``, ``margin_minutes`` and ``unreached_safe`` (``BatchedFireSimulation.escape_routes``): ``info["escape_slack"]``
    is then int32 [n_envs, n_agents], how many more ticks every agent may stay where it is and still reach a target cell ahead of the
    fire (2147483647: no deadline binds; -1: no route is left), and ``info["escape_move"]`` int32 [n_envs, n_agents] the move code
    1..4 towards the neighbour with the largest slack (0: no hurry, or lost) - ``time_to_fire`` up to the horizon and
    ``FireEngine.escape``, both from the state the observation shows.  Off by default: calls and ``info`` are
    what they are without it.

    ``components``: ``None``, or a dict with ``select`` (BurnStatus members, names or ints; default BURNING) and ``connectivity``
    (4, 8 or None: the configured ``diagonal_spread``): ``info["fire_count"]`` is then int32 [n_envs], the number of separate fires,
    and ``info["largest_fire_cells"]`` int32 [n_envs] the cells of the largest (``FireEngine.components``), both
    from the state the observation shows.  Off by default: calls and ``info`` are what they are without it.

    Agents are not part of an environment's state: ``clone_envs`` / ``get_state`` / ``set_state`` do not carry them."""

    def __init__(self, sim, n_agents, start_xy, n_updates=1, weights=(-1, 0, 0, 0), only_unburned=True, done_on_burn=False,
                 max_ticks=0, auto_reset=True, obs=None, values=None, value_weight=None, fire_distance=None, reach=None,
                 moves_to=None, behavior=None, time_to_fire=None, perimeter=None, escape=None, components=None):
        self.sim = sim
        self.engine = sim._engine
        self.n_envs, self.n_agents = int(sim.n_envs), int(n_agents)
        if not 1 <= self.n_agents <= 64:
            raise ValueError(f"BatchedFireEnv: {self.n_agents} agents per environment (1..64)")
        s = np.asarray(start_xy)
        if s.dtype.kind not in "iu":
            raise ValueError(f"BatchedFireEnv: start_xy must be integers, got {s.dtype}")
        if s.shape == (self.n_agents, 2):
            s = np.broadcast_to(s, (self.n_envs, self.n_agents, 2))
        if s.shape != (self.n_envs, self.n_agents, 2):
            raise ValueError(f"BatchedFireEnv: start_xy must have shape {(self.n_agents, 2)} or {(self.n_envs, self.n_agents, 2)}, got {s.shape}")
        self.start_xy = np.ascontiguousarray(s, dtype=np.int32)
        self.obs_kwargs = dict(obs) if obs is not None else dict(channels=["fire_map", "agent_positions"])
        if "channels" not in self.obs_kwargs:
            raise ValueError("BatchedFireEnv: obs needs channels")
        if "agents" in self.obs_kwargs or "envs" in self.obs_kwargs:
            raise ValueError("BatchedFireEnv: obs takes the agents from the device and always shows every environment")
        self.fire_distance = None
        if fire_distance is not None:
            if not isinstance(fire_distance, dict) or set(fire_distance) - {"status", "max_dist"}:
                raise ValueError("BatchedFireEnv: fire_distance is None or a dict of status and max_dist")
            self.fire_distance = dict(status=fire_distance.get("status", ("BURNING",)), max_dist=fire_distance.get("max_dist"))
            sim._engine._distance_request(**self.fire_distance)       # (raises on a bad status or cap before anything is created)
        self.reach = None
        if reach is not None:
            if not isinstance(reach, dict) or set(reach) - {"source", "through", "connectivity", "value"}:
                raise ValueError("BatchedFireEnv: reach is None or a dict of source, through, connectivity and value")
            if not isinstance(reach.get("value", False), bool):
                raise ValueError("BatchedFireEnv: reach's value is True or False")
            self.reach = dict(source=reach.get("source", ("BURNING",)), through=reach.get("through", ("UNBURNED",)),
                              connectivity=reach.get("connectivity"), value=reach.get("value", False))
            sim._engine._reach_request(self.reach["source"], self.reach["through"], self.reach["connectivity"])      # (raises before anything is created)
            if self.reach["value"] and values is None and not self.engine.values_on:
                raise ValueError("BatchedFireEnv: reach's value needs values (or a value plane set on the simulation)")
        self.moves_to = None
        if moves_to is not None:
            if not isinstance(moves_to, dict) or set(moves_to) - {"target", "through", "passable", "targets", "max_moves"}:
                raise ValueError("BatchedFireEnv: moves_to is None or a dict of target, through, passable, targets and max_moves")
            self.moves_to = dict(target=moves_to.get("target", ("BURNING",)), through=moves_to.get("through", ("UNBURNED",)),
                                 passable=moves_to.get("passable"), targets=moves_to.get("targets"), max_moves=moves_to.get("max_moves"))
            from . import walk                                      # (raises before anything is created)
            try:
                walk.request(self.moves_to["target"], self.moves_to["through"], 4, self.moves_to["max_moves"],
                             targets=self.moves_to["targets"] is not None)
            except ValueError as err:
                raise ValueError(f"BatchedFireEnv: moves_to: {err}") from None
        self.time_to_fire = None
        if time_to_fire is not None:
            if not isinstance(time_to_fire, dict) or set(time_to_fire) - {"source", "through", "passable", "max_minutes"}:
                raise ValueError("BatchedFireEnv: time_to_fire is None or a dict of source, through, passable and max_minutes")
            self.time_to_fire = dict(source=time_to_fire.get("source", ("BURNING",)), through=time_to_fire.get("through", ("UNBURNED",)),
                                     passable=time_to_fire.get("passable"), max_minutes=time_to_fire.get("max_minutes"))
            from . import travel                                    # (raises before anything is created)
            try:
                travel.request(self.time_to_fire["source"], self.time_to_fire["through"], None, self.time_to_fire["max_minutes"])
            except ValueError as err:
                raise ValueError(f"BatchedFireEnv: time_to_fire: {err}") from None
        self.perimeter = None
        if perimeter is not None:
            if not isinstance(perimeter, dict) or set(perimeter) - {"status"}:
                raise ValueError("BatchedFireEnv: perimeter is None or a dict of status")
            from . import perimeter as _perimeter                   # (raises before anything is created)
            self.perimeter = dict(status=perimeter.get("status", _perimeter.DEFAULT_STATUS))
            try:
                _perimeter.request(self.perimeter["status"])
            except ValueError as err:
                raise ValueError(f"BatchedFireEnv: {err}") from None
        self.escape = None
        if escape is not None:
            keys = {"target", "targets", "through", "passable", "horizon_minutes", "minutes_per_move", "margin_minutes", "unreached_safe"}
            if not isinstance(escape, dict) or set(escape) - keys:
                raise ValueError("BatchedFireEnv: escape is None or a dict of " + ", ".join(sorted(keys)))
            self.escape = dict(target=escape.get("target", ()), targets=escape.get("targets"), through=escape.get("through", ("UNBURNED",)),
                               passable=escape.get("passable"), horizon_minutes=escape.get("horizon_minutes"),
                               minutes_per_move=escape.get("minutes_per_move"), margin_minutes=escape.get("margin_minutes", 0.0),
                               unreached_safe=escape.get("unreached_safe", False))
            from . import escape as _escape                         # (raises before anything is created)
            try:
                _escape.request(self.escape["target"], self.escape["through"], 4,
                                float(self.engine.params.update_rate) if self.escape["minutes_per_move"] is None else self.escape["minutes_per_move"],
                                self.escape["margin_minutes"], self.escape["horizon_minutes"], self.escape["unreached_safe"],
                                targets=self.escape["targets"] is not None)
            except ValueError as err:
                raise ValueError(f"BatchedFireEnv: {err}") from None
        self.components = None
        if components is not None:
            if not isinstance(components, dict) or set(components) - {"select", "connectivity"}:
                raise ValueError("BatchedFireEnv: components is None or a dict of select and connectivity")
            self.components = dict(select=components.get("select", ("BURNING",)), connectivity=components.get("connectivity"))
            from . import components as _components                 # (raises before anything is created)
            try:
                _components.request(self.components["select"], self.components["connectivity"])
            except ValueError as err:
                raise ValueError(f"BatchedFireEnv: {err}") from None
        self.behavior = None
        if behavior is not None:
            if not isinstance(behavior, dict) or set(behavior) - {"flame_limit", "edges", "summary"}:
                raise ValueError("BatchedFireEnv: behavior is None or a dict of flame_limit, edges and summary")
            self.behavior = dict(edges=behavior.get("edges"), summary=behavior.get("summary", ("BURNING",)))
            from . import behavior as _behavior                     # (raises before anything is created)
            try:
                _behavior.request(None, self.behavior["summary"], behavior.get("flame_limit"), self.behavior["edges"])
            except ValueError as err:
                raise ValueError(f"BatchedFireEnv: {err}") from None
        self.engine.agents_create(self.n_agents, sim.ignitions, n_updates=n_updates, weights=weights, only_unburned=only_unburned,
                                  done_on_burn=done_on_burn, max_ticks=max_ticks, auto_reset=auto_reset)
        self.values_on = values is not None
        if value_weight is not None and not (self.values_on or self.engine.values_on):
            raise ValueError("BatchedFireEnv: value_weight needs values (or a value plane set on the simulation)")
        if self.values_on:
            sim.set_values(values)
        self.values_on = self.values_on or value_weight is not None
        if value_weight is not None:
            self.engine.agents_set_value_weight(value_weight)
        self._all = np.arange(self.n_envs, dtype=np.int32)
        self.engine.agents_place(self._all, self.start_xy, also_start=True)      # (raises on a cell off the grid)

    def _observe(self, info=None):
        """The observation, complete: the one wait for the handle's stream of a ``reset`` / ``step`` (the outputs of ``agents_step``
        enqueued before it are complete then, too).  With ``fire_distance`` and an ``info`` dict, the agents' distances are enqueued
        in front of that wait and put into it."""
        obs = self.sim.observe(agents=self.engine.agents_device(), **self.obs_kwargs)
        if info is not None and self.fire_distance is not None:
            info["fire_distance"] = self.engine.distance(points=self.engine.agents_device(), dtype="float32", **self.fire_distance)
        if info is not None and self.reach is not None:
            r = self.engine.reach(points=self.engine.agents_device(), count=True, **self.reach)
            info["reach_cells"], info["agent_exposed"] = r["count"], r["point_in"]
            if self.reach["value"]:
                info["reach_value"] = r["value"]
        if info is not None and self.moves_to is not None:
            r = self.engine.walk(points=self.engine.agents_device(), connectivity=4, step=True, **self.moves_to)
            info["moves_to"], info["move_toward"] = r["point_moves"], r["point_step"]
        if info is not None and self.behavior is not None:
            r = self.engine.behavior(points=self.engine.agents_device(), planes=(), stats=True, **self.behavior)
            info["flame_length"], info["max_flame"] = r["point_flame"], r["max_flame"]
        if info is not None and self.time_to_fire is not None:
            info["minutes_to_fire"] = self.engine.travel(points=self.engine.agents_device(), plane=False, **self.time_to_fire)["point_minutes"]
        if info is not None and self.perimeter is not None:
            r = self.engine.perimeter(**self.perimeter)
            info["fire_perimeter"], info["fire_cells"] = r["edges"], r["cells"]
        if info is not None and self.escape is not None:
            from .simulation import _escape_routes
            r = _escape_routes(self.engine, None, None, dict(points=self.engine.agents_device(), connectivity=4, step=True, **self.escape))
            info["escape_slack"], info["escape_move"] = r["point_slack"], r["point_step"]
        if info is not None and self.components is not None:
            r = self.engine.components(count=True, largest=True, **self.components)
            info["fire_count"], info["largest_fire_cells"] = r["count"], r["largest"][:, 1]
        self.engine.sync()
        return obs

    def reset(self):
        """New episodes everywhere (``sim.reset()``), the agents on their start cells.  While the simulation draws its episodes
        (``sim.randomize_episodes``) they are drawn ones instead (``sim.new_episodes(all=True)``: every environment's next episode
        index), and with an ``agent_box`` the drawn start cells replace ``start_xy`` - the agents are placed first all the same,
        which clears the episode statistics.  Returns the observation."""
        if self.sim.episodes_randomized:
            self.engine.agents_place(self._all, self.start_xy, also_start=True)
            self.sim.new_episodes(all=True)
            return self._observe()
        self.sim.reset()
        self.engine.agents_place(self._all, self.start_xy, also_start=True)
        return self._observe()

    def episode_info(self):
        """``BatchedFireSimulation.episode_info``: what the last draw of every environment made (index of the next episode,
        ignition, wind), as device tensors."""
        return self.sim.episode_info()

    def step(self, actions):
        """``actions``: torch CUDA int32 [n_envs, n_agents] (``action_word``).  Returns ``(obs, reward float32 [n_envs],
        done bool [n_envs], info)`` with ``info = dict(terms int32 [n_envs, 4], final_len int32 [n_envs], final_ret float64
        [n_envs])``: the episode length and return of the environments that are done, else 0.  New tensors every call."""
        import torch
        dev = self.engine.torch_device
        E = self.n_envs
        reward = torch.empty(E, dtype=torch.float32, device=dev)
        done = torch.empty(E, dtype=torch.bool, device=dev)
        terms = torch.empty((E, 4), dtype=torch.int32, device=dev)
        final_len = torch.empty(E, dtype=torch.int32, device=dev)
        final_ret = torch.empty(E, dtype=torch.float64, device=dev)
        self.engine.agents_step(actions, reward=reward, done=done, terms=terms, final_len=final_len, final_ret=final_ret)
        info = dict(terms=terms, final_len=final_len, final_ret=final_ret)
        obs = self._observe(info)
        if self.values_on:
            info["value_lost"] = self.engine.values_torch()[1]
        return obs, reward, done, info

    def set_wind(self, speed_mph, direction, envs=None):
        """``BatchedFireSimulation.set_wind``: the wind of ``envs`` from the next tick on."""
        self.sim.set_wind(speed_mph, direction, envs)

    def set_wind_schedule(self, envs, segments):
        """``BatchedFireSimulation.set_wind_schedule``: a tick runs under the wind of its environments' update counts at its start; an
        episode restarted inside ``step`` is under its schedule's first row from the next ``step`` on."""
        self.sim.set_wind_schedule(envs, segments)

    def ignite(self, points):
        """``BatchedFireSimulation.ignite``: rows ``(env, column, row)``, NumPy or a CUDA tensor - new fire from the next tick on.
        A CUDA tensor written on torch's current stream (a policy's output) needs no ordering by the caller: that stream is waited
        for before the rows are read; other torch streams are the caller's to order.  Not an agent action: the action words stay
        what they are."""
        self.sim.ignite(points)

    def positions(self):
        """torch int32 [n_envs, n_agents, 3] = (column, row, id): a view of the device positions (current after ``reset`` / ``step``,
        which wait for the handle's stream)."""
        return self.engine.agents_device()

    def close(self):
        self.engine.agents_create(0)
