"""Reference for ignitions during an episode (``sf_ignite``), independent of the library: a thin wrapper over
the sprite-list oracle (``oracle.fire_sprites.SpriteFire``) in table mode.

The reference keeps ``sprites`` / ``durations`` as parallel lists (fire.py:102-103, 578-579); after every ``update()`` the list is
ordered by age, oldest first, and inside one age by ``(y, x)`` ascending (``np.unique``, fire.py:566).  An ignition between two
``update()`` calls inserts a sprite of duration 0 at the place that keeps this order and sets ``fire_map[y, x] = BURNING``: the cell
cannot be told from one the last ``update()`` ignited.  Pinned against the real reference by ``tests/golden/ignite_*.npz``
(``tests/golden/make_golden_ignite.py`` inserts real ``Fire`` sprites into the real manager's lists)."""
import numpy as np

from oracle import fire_sprites

UNBURNED, BURNING = fire_sprites.UNBURNED, fire_sprites.BURNING


def canonical_insert(sprites, durations, new_xy):
    """``new_xy`` (distinct (x, y), none in ``sprites``) as duration-0 entries of the parallel lists ``sprites`` ((x, y) tuples) /
    ``durations``: merged into the trailing duration-0 group, which is then sorted by (y, x).  Returns the new lists."""
    k = len(durations)
    while k > 0 and durations[k - 1] == 0:
        k -= 1
    assert all(d > 0 for d in durations[:k]), "the list is ordered by age, oldest first"
    young = sorted(list(sprites[k:]) + [tuple(int(v) for v in p) for p in new_xy], key=lambda p: (p[1], p[0]))
    return list(sprites[:k]) + young, list(durations[:k]) + [0] * len(young)


class IgniteFire:
    """One environment: ``SpriteFire`` in table mode + its fire map, update count and arrival plane (the first update a cell showed
    a new sprite, -1 = never; 0 = the reset's ignition or an ignition before the first update - ``_arrival_oracle.py``'s count)."""

    def __init__(self, shape, init_pos, rtable, max_fire_duration, pixel_scale, update_rate, max_time=None, attenuate_line_ros=True,
                 diagonal_spread=True):
        self.fire = fire_sprites.SpriteFire(tuple(shape), init_pos, max_fire_duration, pixel_scale, update_rate, rtable=rtable,
                                            max_time=max_time, attenuate_line_ros=attenuate_line_ros, diagonal_spread=diagonal_spread)
        self.fire_map = np.full(tuple(shape), UNBURNED, dtype=np.int64)
        self.fire_map[init_pos[1], init_pos[0]] = BURNING
        self.steps = 0
        self.running = True
        self.arrival = np.full(tuple(shape), -1, dtype=np.int32)
        self.arrival[init_pos[1], init_pos[0]] = 0

    def ignite(self, points):
        """``points``: (x, y) pairs.  Cells that are not UNBURNED and repeats are skipped; nothing happens once the fire has QUIT.
        Returns the cells lit, in the order given."""
        if not self.running:
            return []
        lit = []
        for x, y in points:
            x, y = int(x), int(y)
            if self.fire_map[y, x] == UNBURNED and (x, y) not in lit:
                lit.append((x, y))
        f = self.fire
        f.sprites, f.durations = canonical_insert(f.sprites, f.durations, lit)
        for x, y in lit:
            self.fire_map[y, x] = BURNING
            if self.arrival[y, x] < 0:
                self.arrival[y, x] = self.steps
        return lit

    def apply_mitigation(self, points):
        fire_sprites.apply_mitigation(self.fire_map, points)

    def update(self):
        """One ``update()`` while RUNNING (the loop of ``FireSimulation.run``); returns whether the fire is still running."""
        if not self.running:
            return False
        before = self.fire_map == BURNING
        self.fire_map, st = self.fire.update(self.fire_map)
        self.steps += 1
        self.running = st == fire_sprites.RUNNING
        new = (self.fire_map == BURNING) & ~before & (self.arrival < 0)
        self.arrival[new] = self.steps
        return self.running

    def counts(self):
        """The result row of ``sf_get_status``: running, update() calls made, cells per BurnStatus 0..5."""
        return [int(self.running), self.steps] + [int((self.fire_map == s).sum()) for s in range(6)]
