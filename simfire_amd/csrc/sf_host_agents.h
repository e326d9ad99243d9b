// Host code of the agents and the drawn episodes (section 19).
// Part of the single translation unit simfire_hip.hip (included there, behind sf_handle.h).
#pragma once

// ----------------------------------------------------------------------------- agents
static int agents_free(sf_sim *s)
{
    if (s->agents.mem) {
        HIPCHK(hipStreamSynchronize(s->stream));      // (enqueued ticks may still use the buffers)
        s->bytes -= (int64_t)s->agents.bytes;
    }
    HIPCHK(s->agents.release());
    s->agents.has_ign = false;
    s->values.w_on = false;                              // (the fifth weight belongs to the agent state: set again behind sf_agents_create)
    memset(&s->agents.p, 0, sizeof s->agents.p);
    return SF_OK;
}

extern "C" int sf_agents_create(sf_sim *s, const sf_agent_params *p, const int32_t *ignitions_xy)
{
    if (!s || !p) return fail(SF_EINVAL, "sf_agents_create: null argument");
    const Geo &g = s->g;
    if (p->k < 0 || p->k > kAgentsMax) return fail(SF_EINVAL, "sf_agents_create: %d agents per environment (1..%d; 0 frees)", p->k, kAgentsMax);
    if (p->k > 0) {
        if (p->n_updates < 1) return fail(SF_EINVAL, "sf_agents_create: n_updates = %d must be >= 1", p->n_updates);
        if (p->max_ticks < 0) return fail(SF_EINVAL, "sf_agents_create: max_ticks = %d must be >= 0", p->max_ticks);
        if (p->auto_reset && !ignitions_xy) return fail(SF_EINVAL, "sf_agents_create: auto_reset needs the ignitions");
        for (int e = 0; ignitions_xy && e < g.E; ++e)
            if (ignitions_xy[2 * e] < 0 || ignitions_xy[2 * e] >= g.W || ignitions_xy[2 * e + 1] < 0 || ignitions_xy[2 * e + 1] >= g.H)
                return fail(SF_EINVAL, "sf_agents_create: ignition (%d, %d) of environment %d is outside the %dx%d grid", ignitions_xy[2 * e],
                            ignitions_xy[2 * e + 1], e, g.H, g.W);
    }
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    SF_TRY(agents_free(s));
    if (p->k == 0) return SF_OK;
    // one allocation, every buffer on a 16-byte boundary: xyid | start | points | prev | terms | len | ign | ret | done
    const size_t E = (size_t)g.E, K = (size_t)p->k;
    const size_t sizes[9] = {E * K * 12, E * K * 8, E * K * 12, E * 4, E * 16, E * 4, E * 8, E * 8, E};
    size_t off[9], total = 0;
    for (int i = 0; i < 9; ++i) { off[i] = total; total += (sizes[i] + 15) / 16 * 16; }
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->agents.mem), total));
    s->agents.bytes = total; s->bytes += (int64_t)total;
    int32_t **ip[7] = {&s->agents.xyid, &s->agents.start, &s->agents.points, &s->agents.prev, &s->agents.terms, &s->agents.len, &s->agents.ign};
    for (int i = 0; i < 7; ++i) *ip[i] = reinterpret_cast<int32_t *>(s->agents.mem + off[i]);
    s->agents.ret = reinterpret_cast<double *>(s->agents.mem + off[7]);
    s->agents.done = s->agents.mem + off[8];
    std::vector<uint8_t> h(total, 0);
    int32_t *xyid = reinterpret_cast<int32_t *>(h.data() + off[0]);
    for (size_t i = 0; i < E * K; ++i) xyid[3 * i + 2] = (int32_t)(i % K) + 1;
    if (ignitions_xy) memcpy(h.data() + off[6], ignitions_xy, E * 8);
    HIPCHK(hipMemcpyAsync(s->agents.mem, h.data(), total, hipMemcpyHostToDevice, s->stream));
    // (section 19: episodes that draw no ignition re-ignite where these agents' environments do)
    if (ignitions_xy && s->episodes.on && !(s->episodes.p.flags & SF_EP_IGNITION)) HIPCHK(hipMemcpyAsync(s->episodes.ign, ignitions_xy, E * 8, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));          // (h is pageable and leaves scope)
    s->agents.p = *p;
    s->agents.has_ign = ignitions_xy != nullptr;
    return SF_OK;
}

extern "C" int sf_agents_place(sf_sim *s, int32_t n, const int32_t *envs, const int32_t *xy, int32_t also_start)
{
    if (!s) return fail(SF_EINVAL, "sf_agents_place: null handle");
    if (!s->agents.p.k) return fail(SF_ESTATE, "sf_agents_place: call sf_agents_create first");
    if (n < 0 || (n > 0 && (!envs || !xy))) return fail(SF_EINVAL, "sf_agents_place: bad environment list");
    const Geo &g = s->g;
    const int K = s->agents.p.k;
    SF_TRY(check_envs(s, "sf_agents_place", n, envs));
    for (long long i = 0; i < (long long)n * K; ++i)
        if (xy[2 * i] < 0 || xy[2 * i] >= g.W || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= g.H)
            return fail(SF_EINVAL, "sf_agents_place: cell (%d, %d) of agent %d of environment %d is outside the %dx%d grid", xy[2 * i],
                        xy[2 * i + 1], (int)(i % K), envs[i / K], g.H, g.W);
    if (n == 0) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    // an environment named twice keeps its last entry: no two threads of the launch write one agent
    std::vector<int32_t> last((size_t)g.E, -1), keep;
    for (int i = 0; i < n; ++i) last[envs[i]] = i;
    for (int i = 0; i < n; ++i) if (last[envs[i]] == i) keep.push_back(i);
    const int m = (int)keep.size();
    // the call block: envs [m] | xy [m][K][2]
    const size_t o_xy = ((size_t)m * 4 + 15) / 16 * 16, bytes = o_xy + (size_t)m * K * 8;
    CallBlock &blk = s->agents.blk;
    SF_TRY(block_reserve(s, blk, bytes));
    for (int i = 0; i < m; ++i) {
        reinterpret_cast<int32_t *>(blk.pinned)[i] = envs[keep[i]];
        memcpy(blk.pinned + o_xy + (size_t)i * K * 8, xy + (size_t)keep[i] * K * 2, (size_t)K * 8);
    }
    SF_TRY(block_send(s, blk, bytes));
    hipLaunchKernelGGL(k_agents_place, dim3((unsigned)((m * K + 255) / 256)), dim3(256), 0, s->stream, m, K,
                       reinterpret_cast<const int32_t *>(blk.dev), reinterpret_cast<const int32_t *>(blk.dev + o_xy), also_start != 0 ? 1 : 0,
                       s->agents.xyid, s->agents.start, s->agents.len, s->agents.ret);
    HIPCHK(hipGetLastError());
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_agents_device(sf_sim *s, void **xyid)
{
    if (!s || !xyid) return fail(SF_EINVAL, "sf_agents_device: null argument");
    if (!s->agents.p.k) return fail(SF_ESTATE, "sf_agents_device: call sf_agents_create first");
    *xyid = s->agents.xyid;
    return SF_OK;
}


// ----------------------------------------------------------------------------- drawn episodes
static int episodes_free(sf_sim *s)
{
    if (s->episodes.mem) {
        HIPCHK(hipStreamSynchronize(s->stream));      // (enqueued ticks may still use the buffers)
        s->bytes -= (int64_t)s->episodes.bytes;
    }
    HIPCHK(s->episodes.release());
    memset(&s->episodes.p, 0, sizeof s->episodes.p);
    s->episodes.on = false;
    return SF_OK;
}

// New episodes in the environments the mask takes (null: those that are not running), their parameters drawn first (enqueue layer):
// the draw, the batched reset with the drawn ignitions, then - SF_EP_WIND - the tables of the drawn winds, so that the episode runs
// under its own wind from its first update.  Nothing is read back.
static int episode_begin(sf_sim *s, const uint8_t *mask)
{
    const Geo &g = s->g;
    const sf_episode_params &p = s->episodes.p;
    const bool wind = (p.flags & SF_EP_WIND) != 0;
    bool cached = false;
    if (wind) {
        // the cache of wind-independent terms current for EVERY table (which ones restart is known on the device only), again after
        // anything staled a part of it (TableBook); without a cache the tables are built from the layers
        const int n_tab = s->tables.size();
        const bool stale = !s->wind.terms || s->wind.cache_off || s->tables.any_wt_stale();
        cached = !stale;
        if (stale && !s->episodes.nocache) {
            const int rc = ensure_wterms(s, iota_tabs(0, n_tab).data(), n_tab);
            if (rc && rc != SF_ENOTSUP) return rc;
            cached = rc == SF_OK;
            s->episodes.nocache = !cached;
        }
    }
    EpisodeArgs a;
    memset(&a, 0, sizeof a);
    a.H = g.H; a.W = g.W; a.P = g.P; a.E = g.E;
    a.mask = mask; a.commit = s->commit;
    a.seed = p.seed; a.flags = p.flags;
    for (int i = 0; i < 4; ++i) { a.ign_box[i] = p.ign_box[i]; a.agent_box[i] = p.agent_box[i]; }
    for (int i = 0; i < 2; ++i) { a.U[i] = p.U[i]; a.U_dir[i] = p.U_dir[i]; }
    a.rt = s->rt; a.tab_stride = (size_t)s->tables.size() > 1 ? (long long)8 * g.plane_env : 0;
    a.index = s->episodes.index; a.ign = s->episodes.ign; a.wind = s->episodes.wind;
    a.K = (p.flags & SF_EP_AGENTS) ? s->agents.p.k : 0;
    a.start = s->agents.start; a.xyid = s->agents.xyid;
    a.due_cnt = s->episodes.due_cnt; a.due = s->episodes.due; a.due_U = s->episodes.due_U; a.due_D = s->episodes.due_D;
    if (wind) HIPCHK(hipMemsetAsync(s->episodes.due_cnt, 0, sizeof(uint32_t), s->stream));
    hipLaunchKernelGGL(k_episode_draw, dim3((unsigned)g.E), dim3(kEpAttempts), 0, s->stream, a);
    HIPCHK(hipGetLastError());
    SF_TRY(reset_launch(s, nullptr, mask, s->episodes.ign, g.E));
    // (section 15's bookkeeping of the mask form: which environments were taken is known on the device only)
    if (s->delta.snap) std::fill(s->delta.snap_valid.begin(), s->delta.snap_valid.end(), 0);
    if (wind) {
        SF_TRY(wind_launch(s, s->episodes.due, s->episodes.due_cnt, 0, g.E, s->episodes.due_U, s->episodes.due_D, 0, cached));
        // (the cell-major copies as in sf_set_wind: where the buffer exists the pass has written the listed tables' copies too - a copy
        // that was stale is no worse for it; where it does not, every copy is stale until ensure_rtc has built it)
    }
    return SF_OK;
}

extern "C" int sf_episodes_set(sf_sim *s, const sf_episode_params *p)
{
    const char *who = "sf_episodes_set";
    if (!s) return fail(SF_EINVAL, "%s: null handle", who);
    const Geo &g = s->g;
    if (p) {
        if (p->flags & ~(SF_EP_IGNITION | SF_EP_LIVE_CELL | SF_EP_WIND | SF_EP_AGENTS)) return fail(SF_EINVAL, "%s: unknown flags 0x%x", who, p->flags);
        if (p->reserved != 0) return fail(SF_EINVAL, "%s: reserved must be 0", who);
        if ((p->flags & SF_EP_LIVE_CELL) && !(p->flags & SF_EP_IGNITION)) return fail(SF_EINVAL, "%s: SF_EP_LIVE_CELL needs SF_EP_IGNITION", who);
        const struct { int flag; const int32_t *box; const char *name; } boxes[2] = {{SF_EP_IGNITION, p->ign_box, "ign_box"}, {SF_EP_AGENTS, p->agent_box, "agent_box"}};
        for (const auto &b : boxes)
            if ((p->flags & b.flag) && (b.box[0] < 0 || b.box[1] < 0 || b.box[2] >= g.W || b.box[3] >= g.H || b.box[0] > b.box[2] || b.box[1] > b.box[3]))
                return fail(SF_EINVAL, "%s: %s (%d, %d, %d, %d) is not x0 <= x1, y0 <= y1 on the %dx%d grid", who, b.name, b.box[0], b.box[1], b.box[2], b.box[3], g.H, g.W);
        if (p->flags & SF_EP_WIND) {
            const bool ok = std::isfinite(p->U[0]) && std::isfinite(p->U[1]) && std::isfinite(p->U_dir[0]) && std::isfinite(p->U_dir[1]) &&
                            p->U[0] >= 0.0 && p->U[0] <= p->U[1] && p->U_dir[0] <= p->U_dir[1];
            if (!ok) return fail(SF_EINVAL, "%s: wind ranges U [%g, %g], U_dir [%g, %g] must be finite with lo <= hi and U >= 0", who, p->U[0], p->U[1], p->U_dir[0], p->U_dir[1]);
            if (!s->p.per_env_terrain) return fail(SF_ESTATE, "%s: SF_EP_WIND: this handle shares one terrain between all environments (create it with per_env_terrain = 1)", who);
            for (int t = 0; t < s->tables.size(); ++t)
                if (!s->tables[t].layers) return fail(SF_ESTATE, "%s: SF_EP_WIND: table %d has no layers (sf_set_layers*, sf_generate_layers)", who, t);
            if (!s->wind.sched.empty()) return fail(SF_ESTATE, "%s: SF_EP_WIND while a wind schedule is set (sf_set_wind_schedule): the two would fight over the table", who);
        }
        if (!(p->flags & SF_EP_IGNITION) && !(s->agents.p.k && s->agents.has_ign) && s->last_ign.empty())
            return fail(SF_ESTATE, "%s: without SF_EP_IGNITION new episodes ignite where the environment last did: call sf_reset or sf_agents_create (with ignitions) first", who);
    }
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    SF_TRY(episodes_free(s));
    if (!p) return SF_OK;
    // one allocation, every buffer on a 16-byte boundary: index | ign | wind | due | due_cnt | due_U | due_D | ones
    const size_t E = (size_t)g.E;
    const size_t sizes[8] = {E * 4, E * 8, E * 16, E * 4, 4, E * 8, E * 8, E};
    size_t off[8], total = 0;
    for (int i = 0; i < 8; ++i) { off[i] = total; total += (sizes[i] + 15) / 16 * 16; }
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->episodes.mem), total));
    s->episodes.bytes = total; s->bytes += (int64_t)total;
    s->episodes.index = reinterpret_cast<uint32_t *>(s->episodes.mem + off[0]);
    s->episodes.ign = reinterpret_cast<int32_t *>(s->episodes.mem + off[1]);
    s->episodes.wind = reinterpret_cast<double *>(s->episodes.mem + off[2]);
    s->episodes.due = reinterpret_cast<int32_t *>(s->episodes.mem + off[3]);
    s->episodes.due_cnt = reinterpret_cast<uint32_t *>(s->episodes.mem + off[4]);
    s->episodes.due_U = reinterpret_cast<double *>(s->episodes.mem + off[5]);
    s->episodes.due_D = reinterpret_cast<double *>(s->episodes.mem + off[6]);
    s->episodes.ones = s->episodes.mem + off[7];
    std::vector<uint8_t> h(total, 0);
    memset(h.data() + off[7], 1, E);
    const bool from_agents = s->agents.p.k && s->agents.has_ign;
    if (!(p->flags & SF_EP_IGNITION) && !from_agents) memcpy(h.data() + off[1], s->last_ign.data(), E * 8);
    HIPCHK(hipMemcpyAsync(s->episodes.mem, h.data(), total, hipMemcpyHostToDevice, s->stream));
    if (!(p->flags & SF_EP_IGNITION) && from_agents) HIPCHK(hipMemcpyAsync(s->episodes.ign, s->agents.ign, E * 8, hipMemcpyDeviceToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));          // (h is pageable and leaves scope)
    s->episodes.p = *p;
    s->episodes.on = true;
    s->episodes.nocache = false;
    return SF_OK;
}

extern "C" int sf_episodes_begin(sf_sim *s, const uint8_t *device_mask, int32_t all)
{
    const char *who = "sf_episodes_begin";
    if (!s) return fail(SF_EINVAL, "%s: null handle", who);
    if (!s->episodes.on) return fail(SF_ESTATE, "%s: call sf_episodes_set first", who);
    const bool tables = (s->episodes.p.flags & (SF_EP_LIVE_CELL | SF_EP_WIND)) != 0;      // the draw reads, or the wind pass rebuilds, R tables
    SF_TRY(begin_call(s, who, kStateCall | (tables ? kNeedRt : 0)));
    SF_TRY(episode_begin(s, all ? s->episodes.ones : device_mask));
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_episodes_device(sf_sim *s, void **index, void **ignition, void **wind)
{
    if (!s) return fail(SF_EINVAL, "sf_episodes_device: null handle");
    if (!index || !ignition || !wind) return fail(SF_EINVAL, "sf_episodes_device: null argument");
    if (!s->episodes.on) return fail(SF_ESTATE, "sf_episodes_device: call sf_episodes_set first");
    *index = s->episodes.index; *ignition = s->episodes.ign; *wind = s->episodes.wind;
    return SF_OK;
}

static AgentArgs agent_args(const sf_sim *s, const int32_t *actions, const sf_agent_out *out)
{
    AgentArgs a;
    memset(&a, 0, sizeof a);
    a.g = s->g;
    a.pl = cur_planes(s);          // (whichever plane is current NOW: the step between the two kernels may change it)
    a.rows = s->status_block;
    a.actions = actions;
    a.xyid = s->agents.xyid; a.start = s->agents.start; a.points = s->agents.points; a.prev_cnt = s->agents.prev; a.terms = s->agents.terms;
    a.ep_len = s->agents.len; a.ep_ret = s->agents.ret; a.done = s->agents.done;
    a.K = s->agents.p.k; a.only_unburned = s->agents.p.only_unburned != 0; a.done_on_burn = s->agents.p.done_on_burn != 0;
    a.max_ticks = s->agents.p.max_ticks; a.auto_reset = s->agents.p.auto_reset != 0;
    for (int i = 0; i < 4; ++i) a.w[i] = (double)s->agents.p.w[i];
    if (s->values.plane) {
        a.damage = s->values.aux; a.damage_stride = (long long)sizeof(ValueRec);
        a.tick_base = s->val_tick(0); a.tick_loss = s->val_tick(1);
        a.wv = (double)s->values.w; a.wv_on = s->values.w_on ? 1 : 0;
    }
    if (out) { a.o_reward = out->reward; a.o_done = out->done; a.o_terms = out->terms; a.o_len = out->final_len; a.o_ret = out->final_ret; }
    return a;
}

// One tick for every environment, nothing read back, every piece from the enqueue layer: result rows -> k_agents_act -> one update
// with the device points, then the plain updates -> result rows -> k_agents_finish -> the batched reset with the done mask.
extern "C" int sf_agents_step(sf_sim *s, const int32_t *device_actions, const sf_agent_out *out)
{
    if (!s) return fail(SF_EINVAL, "sf_agents_step: null handle");
    if (!s->agents.p.k) return fail(SF_ESTATE, "sf_agents_step: call sf_agents_create first");
    if (!device_actions) return fail(SF_EINVAL, "sf_agents_step: null actions");
    const Geo &g = s->g;
    SF_TRY(begin_call(s, "sf_agents_step", kNeedRt | kStateCall));
    note_result_look(s);
    int rc = refresh_status(s, nullptr);             // r0: the rows as a status query leaves them
    const int32_t *pts = nullptr;
    if (!rc) rc = stage_lines(s, 1, s->agents.points, s->agents.p.k, 1, &pts);
    if (!rc) {
        hipLaunchKernelGGL(k_agents_act, dim3((unsigned)g.E), dim3(kAgentsMax), 0, s->stream, agent_args(s, device_actions, out));
        const StepPlan plan = plan_step(s, 1, true);         // one update with the device points: inside the resident launch, or a pair
        rc = plan.nw ? enqueue_call(s, plan, 1, pts, s->agents.p.k, false, nullptr) : enqueue_pair(s, pts, s->agents.p.k, 0, nullptr);
        if (!rc && s->arrival.pending) rc = arrival_pass(s);
    }
    if (!rc) rc = step_impl(s, s->agents.p.n_updates - 1, false, nullptr);
    if (!rc) { note_result_look(s); rc = refresh_status(s, nullptr); }      // r1 (commits the step rings too)
    if (!rc) {
        hipLaunchKernelGGL(k_agents_finish, dim3((unsigned)g.E), dim3(kAgentsMax), 0, s->stream, agent_args(s, device_actions, out));
        if (s->agents.p.auto_reset && s->episodes.on) rc = episode_begin(s, s->agents.done);      // section 19: the new episodes are drawn
        else if (s->agents.p.auto_reset) {
            rc = reset_launch(s, nullptr, s->agents.done, s->agents.ign, g.E);
            // (section 15's bookkeeping of the mask form: which environments were taken is known on the device only)
            if (!rc && s->delta.snap) std::fill(s->delta.snap_valid.begin(), s->delta.snap_valid.end(), 0);
        }
    }
    return rc ? rc : finish_call(s, "sf_agents_step", !s->async, nullptr);
}
