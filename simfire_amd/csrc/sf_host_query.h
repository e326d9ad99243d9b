// Host code of the queries: sf_distance, sf_reach (23), sf_walk (24), sf_behavior (25), sf_travel (26), sf_perimeter (27), sf_influence (28), sf_escape (30) and sf_components (31).  Each takes a list
// of environments, optional points and caller-owned device outputs, reads the state and changes none of it.  Included once from
// simfire_hip.hip, behind sf_host_views.h.
//
// The host frame of a query, in this order: null and argument refusals (SF_EINVAL), the environment list, the grid's width
// (SF_ENOTSUP), check_ready (SF_ESTATE), the feature's own SF_ESTATE, begin_call; a list of none ends there.  Then the scratch of as
// many environments as the budget holds (query_chunk, scratch_reserve), the list through the feature's call block, and the launches
// chunk by chunk.  All of it on the handle's stream, so a chunk's launches follow the chunk before it; a refused call has enqueued
// nothing.
#pragma once

// ----------------------------------------------------------------------------- what the queries share
// k and points.  `stray`: points given with k == 0 are refused too (sf_walk and sf_behavior; sf_distance and sf_reach ignore them).
static int check_points(const char *who, int k, const void *points, bool stray)
{
    if (k < 0 || k > SF_DIST_MAX_POINTS) return fail(SF_EINVAL, "%s: %d points per environment (0..%d)", who, k, SF_DIST_MAX_POINTS);
    if (k > 0 && !points) return fail(SF_EINVAL, "%s: k = %d needs points", who, k);
    if (stray && k == 0 && points) return fail(SF_EINVAL, "%s: points need k > 0", who);
    return SF_OK;
}
static int check_reserved(const char *who, int reserved)
{
    return reserved ? fail(SF_EINVAL, "%s: reserved must be 0", who) : SF_OK;
}
// low_bits: the low address bits of every output or'ed, masked by the element's alignment
static int check_aligned(const char *who, uintptr_t low_bits)
{
    return low_bits ? fail(SF_EINVAL, "%s: an output is not aligned to its element", who) : SF_OK;
}
// a budget of the caller's holds one environment's scratch (`what` names it: "plane", "need")
static int check_scratch(const char *who, int64_t scratch_bytes, size_t need, const char *what)
{
    if (scratch_bytes < 0 || (scratch_bytes > 0 && (size_t)scratch_bytes < need))
        return fail(SF_EINVAL, "%s: scratch_bytes %lld is less than one environment's %s (%zu bytes)", who, (long long)scratch_bytes, what, need);
    return SF_OK;
}

// A status mask as the table of one byte permute: byte s of (hi : lo) = 1 if the mask selects BurnStatus s (read by mask_sel01, sf_query_dev.h)
static void mask_tables(int mask, uint32_t &lo, uint32_t &hi)
{
    lo = hi = 0;
    for (int st = 0; st < 6; ++st)
        if ((mask >> st) & 1) (st < 4 ? lo : hi) |= 1u << (8 * (st & 3));
}

// Environments per chunk of a list of n: as many as the budget holds of `need` bytes each, one at least, `cap` (the launch grid) at most
static int query_chunk(int n, int64_t scratch_bytes, long long budget_default, size_t need, size_t cap)
{
    const size_t budget = scratch_bytes > 0 ? (size_t)scratch_bytes : (size_t)budget_default;
    return (int)std::min<size_t>({(size_t)n, std::max<size_t>(budget / need, 1), cap});
}

// ----------------------------------------------------------------------------- distance fields
// Per chunk the two column passes over the scratch plane g and k_dist_rows (plane form) or k_dist_points.
extern "C" int sf_distance(sf_sim *s, const sf_dist_params *p, int32_t n, const int32_t *envs, void *device_out)
{
    const char *who = "sf_distance";
    if (!s || !p) return fail(SF_EINVAL, "sf_distance: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && (!envs || !device_out))) return fail(SF_EINVAL, "sf_distance: bad environment list or output");
    if (p->status_mask < 1 || p->status_mask > 63) return fail(SF_EINVAL, "sf_distance: status_mask %d (bit s selects BurnStatus s: 1..63)", p->status_mask);
    if (p->max_d2 < 0) return fail(SF_EINVAL, "sf_distance: max_d2 %d (0: no cap)", p->max_d2);
    if (p->dtype != SF_DIST_I32 && p->dtype != SF_DIST_F32) return fail(SF_EINVAL, "sf_distance: dtype %d (0 int32, 1 float32)", p->dtype);
    SF_TRY(check_points(who, p->k, p->points, false));
    if (!std::isfinite(p->scale) || !(p->scale > 0.0)) return fail(SF_EINVAL, "sf_distance: scale must be finite and > 0");
    SF_TRY(check_reserved(who, p->reserved[0] | p->reserved[1]));
    if ((uintptr_t)device_out & 3) return fail(SF_EINVAL, "sf_distance: the output is not aligned to its element");
    const size_t plane = (size_t)g.plane_env * sizeof(uint16_t);          // one environment's g
    SF_TRY(check_scratch(who, p->scratch_bytes, plane, "plane"));
    SF_TRY(check_envs(s, who, n, envs));
    if ((long long)(g.H - 1) * (g.H - 1) + (long long)(g.W - 1) * (g.W - 1) >= (long long)SF_DIST_FAR)
        return fail(SF_ENOTSUP, "sf_distance: squared distances on a %d x %d grid do not fit int32", g.H, g.W);
    if (g.W > kDistMaxWidth) return fail(SF_ENOTSUP, "sf_distance: grids wider than %d cells are not supported (width %d)", kDistMaxWidth, g.W);
    SF_TRY(begin_call(s, who, kNeedRt | kNeedReset | kNotVoid));
    if (n == 0) return SF_OK;

    const int chunk = query_chunk(n, p->scratch_bytes, kDistScratchDefault, plane, 32768);      // (32768: the launch grid's y)
    QueryState &d = s->dist;
    SF_TRY(scratch_reserve(s, d, (size_t)chunk * plane));
    const int32_t *envs_dev = nullptr;
    SF_TRY(block_stage(s, d.blk, &envs_dev, envs, (size_t)n * sizeof(int32_t)));

    DistArgs a;
    memset(&a, 0, sizeof a);
    a.g = g;
    a.pl = cur_planes(s);
    a.gp = reinterpret_cast<uint16_t *>(d.mem);
    a.k = p->k;
    mask_tables(p->status_mask, a.tlo, a.thi);
    a.limit = p->max_d2 > 0 ? p->max_d2 : SF_DIST_FAR;
    a.reach = g.W;
    if (p->max_d2 > 0) {
        a.reach = (int)std::sqrt((double)p->max_d2);
        while ((long long)a.reach * a.reach < p->max_d2) a.reach++;
        a.reach = std::min(a.reach, g.W);
    }
    a.f32 = p->dtype == SF_DIST_F32;
    a.scale = p->scale;
    a.vec = g.W % 4 == 0 && !((uintptr_t)device_out & 15);
    a.rows = std::max(1, std::min({1024 / g.P, kDistMaxRows, g.H}));
    const size_t per_env = (p->k ? (size_t)p->k : (size_t)g.H * g.W) * 4;      // output bytes per listed environment
    for (int c0 = 0; c0 < n; c0 += chunk) {
        a.cn = std::min(chunk, n - c0);
        a.envs = envs_dev + c0;
        a.out = static_cast<uint8_t *>(device_out) + (size_t)c0 * per_env;
        a.points = p->k ? p->points + (size_t)c0 * p->k * 3 : nullptr;
        const unsigned col_blocks = (unsigned)(((long long)a.cn * g.PV + kDistColsThreads - 1) / kDistColsThreads);
        hipLaunchKernelGGL(k_dist_cols_down, dim3(col_blocks), dim3(kDistColsThreads), 0, s->stream, a);
        hipLaunchKernelGGL(k_dist_cols_up, dim3(col_blocks), dim3(kDistColsThreads), 0, s->stream, a);
        if (p->k)
            hipLaunchKernelGGL(k_dist_points, dim3((unsigned)((p->k + kDistRowsThreads / 64 - 1) / (kDistRowsThreads / 64)), (unsigned)a.cn),
                               dim3(kDistRowsThreads), 0, s->stream, a);
        else
            hipLaunchKernelGGL(k_dist_rows, dim3((unsigned)((g.H + a.rows - 1) / a.rows), (unsigned)a.cn), dim3(kDistRowsThreads),
                               (size_t)a.rows * g.P * sizeof(int32_t), s->stream, a);
    }
    return finish_call(s, who, !s->async, nullptr);
}

// ----------------------------------------------------------------------------- band searches: sf_reach and sf_walk (DESIGN.md sections 23, 24)
// What k_reach and k_walk read alike (both Args begin with a BandArgs, `band`): the state, the passable plane, the two masks
// (`seed_mask`: where the search starts - sources, targets), the points' count, the connectivity and the band geometry.
static void band_args(const sf_sim *s, BandArgs &r, const uint8_t *passable, int per_env, int k, int seed_mask, int through_mask, int conn8)
{
    const Geo &g = s->g;
    r.g = g;
    r.pl = cur_planes(s);
    r.passable = passable;
    r.pass_env = per_env ? (long long)g.H * g.W : 0;
    r.pass_vec = passable && g.W % 16 == 0 && !((uintptr_t)passable & 15);
    r.k = k;
    mask_tables(seed_mask, r.slo, r.shi);
    mask_tables(through_mask, r.tlo, r.thi);
    r.conn8 = conn8;
    r.WORDS = band_words(g.P); r.BR = band_rows(g.H); r.nb = r.BR * r.WORDS;
}

// The launches of a band search and the end of its call: one launch per chunk of as many environments as the budget holds (`need`
// bytes of scratch each), one workgroup per listed environment.  The call block is the environment list | one Args per chunk (the
// kernel takes its arguments from there): `a` with a.band pointed at the chunk's environments and points, and at(c0) having pointed
// the outputs at the part of the chunk that begins with list entry c0.
// One band per thread where the grid allows it: the search's own planes stay in registers and LDS for all of it (k_resident, with
// `lanes` threads rounded up to whole waves); else passes of kBandThreads bands over the scratch planes (k_passes).  Up to 156 KiB
// of LDS at 1024 threads, one workgroup per CU (which 1024 threads are anyway).
template <typename Args, typename At>
static int band_search(sf_sim *s, const char *who, QueryState &q, int32_t n, const int32_t *envs, const int32_t *points, int64_t scratch_bytes,
                       long long budget_default, size_t need, Args &a, At at, void (*k_resident)(const Args *),
                       void (*k_passes)(const Args *), int lanes, size_t (*lds_bytes)(int, bool))
{
    BandArgs &r = a.band;
    const int chunk = query_chunk(n, scratch_bytes, budget_default, need, 65535), chunks = (n + chunk - 1) / chunk;
    SF_TRY(scratch_reserve(s, q, (size_t)chunk * need));
    r.scratch = q.mem;
    r.scratch_env = (long long)need;
    const size_t o_args = ((size_t)n * sizeof(int32_t) + 15) / 16 * 16, bytes = o_args + (size_t)chunks * sizeof(Args);
    SF_TRY(block_reserve(s, q.blk, bytes));
    memcpy(q.blk.pinned, envs, (size_t)n * sizeof(int32_t));
    for (int c = 0; c < chunks; ++c) {
        const int c0 = c * chunk;
        r.envs = reinterpret_cast<const int32_t *>(q.blk.dev) + c0;
        r.points = r.k ? points + (size_t)c0 * r.k * 3 : nullptr;
        at(c0);
        memcpy(q.blk.pinned + o_args + (size_t)c * sizeof(Args), &a, sizeof a);
    }
    SF_TRY(block_send(s, q.blk, bytes));

    const bool resident = r.nb <= kBandThreads;
    const unsigned threads = resident ? (unsigned)((lanes + 63) / 64 * 64) : (unsigned)kBandThreads;
    const size_t lds = lds_bytes((int)threads, resident);
    const auto kernel = resident ? k_resident : k_passes;
    HIPCHK(allow_lds(s, reinterpret_cast<const void *>(kernel), lds));
    for (int c = 0; c < chunks; ++c) {
        const Args *ap = reinterpret_cast<const Args *>(q.blk.dev + o_args) + c;
        hipLaunchKernelGGL(kernel, dim3((unsigned)std::min(chunk, n - c * chunk)), dim3(threads), lds, s->stream, ap);
    }
    return finish_call(s, who, !s->async, nullptr);
}

extern "C" int sf_reach(sf_sim *s, const sf_reach_params *p, int32_t n, const int32_t *envs, const sf_reach_out *out)
{
    const char *who = "sf_reach";
    if (!s || !p || !out) return fail(SF_EINVAL, "sf_reach: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && !envs)) return fail(SF_EINVAL, "sf_reach: bad environment list");
    if (p->source_mask < 1 || p->source_mask > 63) return fail(SF_EINVAL, "sf_reach: source_mask %d (bit s selects BurnStatus s: 1..63)", p->source_mask);
    if (p->through_mask < 1 || p->through_mask > 63) return fail(SF_EINVAL, "sf_reach: through_mask %d (bit s selects BurnStatus s: 1..63)", p->through_mask);
    if (p->source_mask & p->through_mask) return fail(SF_EINVAL, "sf_reach: source_mask %d and through_mask %d overlap", p->source_mask, p->through_mask);
    if (p->connectivity != 0 && p->connectivity != 4 && p->connectivity != 8)
        return fail(SF_EINVAL, "sf_reach: connectivity %d (0: the handle's diagonal_spread, 4, 8)", p->connectivity);
    SF_TRY(check_points(who, p->k, p->points, false));
    if (out->point_in && p->k == 0) return fail(SF_EINVAL, "sf_reach: point_in needs k > 0");
    if (p->max_rounds < 0) return fail(SF_EINVAL, "sf_reach: max_rounds %d (0: to the fixed point)", p->max_rounds);
    SF_TRY(check_reserved(who, p->reserved[0] | p->reserved[1]));
    if (!out->count && !out->value && !out->mask && !out->seeds && !out->point_in && !out->rounds)
        return fail(SF_EINVAL, "sf_reach: every output is null");
    SF_TRY(check_aligned(who, (((uintptr_t)out->count | (uintptr_t)out->seeds | (uintptr_t)out->point_in | (uintptr_t)out->rounds) & 3) | ((uintptr_t)out->value & 7)));
    const size_t need = (size_t)reach_env_bytes(g);
    SF_TRY(check_scratch(who, p->scratch_bytes, need, "need"));
    SF_TRY(check_envs(s, who, n, envs));
    if (g.W > kReachMaxWidth) return fail(SF_ENOTSUP, "sf_reach: grids wider than %d cells are not supported (width %d)", kReachMaxWidth, g.W);
    SF_TRY(check_ready(s, who, kNeedRt | kNeedReset));
    if (out->value && !s->values.plane) return fail(SF_ESTATE, "sf_reach: value needs a value plane (sf_values_set)");
    SF_TRY(begin_call(s, who, kNeedRt | kNeedReset | kNotVoid));
    if (n == 0) return SF_OK;

    ReachArgs a;
    memset(&a, 0, sizeof a);
    band_args(s, a.band, p->passable, p->passable_per_env, p->k, p->source_mask, p->through_mask, p->connectivity == 0 ? g.diag : (p->connectivity == 8));
    a.vals = out->value ? s->values.plane : nullptr;
    a.val_env = s->values.per_env ? g.plane_env : 0;
    a.max_rounds = p->max_rounds;
    a.mask_vec = out->mask && g.W % 16 == 0 && !((uintptr_t)out->mask & 15);
    const auto at = [&](int c0) {
        a.count = out->count ? out->count + c0 : nullptr;
        a.value = out->value ? reinterpret_cast<long long *>(out->value) + c0 : nullptr;
        a.mask = out->mask ? out->mask + (size_t)c0 * g.H * g.W : nullptr;
        a.seeds = out->seeds ? out->seeds + c0 : nullptr;
        a.point_in = out->point_in ? out->point_in + (size_t)c0 * p->k : nullptr;
        a.rounds = out->rounds ? out->rounds + c0 : nullptr;
    };
    return band_search(s, who, s->reach, n, envs, p->points, p->scratch_bytes, kReachScratchDefault, need, a, at, k_reach<true>, k_reach<false>,
                       a.band.nb, reach_lds_bytes);
}

extern "C" int sf_walk(sf_sim *s, const sf_walk_params *p, int32_t n, const int32_t *envs, const sf_walk_out *out)
{
    const char *who = "sf_walk";
    if (!s || !p || !out) return fail(SF_EINVAL, "sf_walk: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && !envs)) return fail(SF_EINVAL, "sf_walk: bad environment list");
    if (p->target_mask < 0 || p->target_mask > 63) return fail(SF_EINVAL, "sf_walk: target_mask %d (bit s selects BurnStatus s: 0..63)", p->target_mask);
    if (p->through_mask < 1 || p->through_mask > 63) return fail(SF_EINVAL, "sf_walk: through_mask %d (bit s selects BurnStatus s: 1..63)", p->through_mask);
    if (p->target_mask == 0 && !p->targets) return fail(SF_EINVAL, "sf_walk: target_mask 0 needs a targets plane");
    if (p->connectivity != 0 && p->connectivity != 4 && p->connectivity != 8)
        return fail(SF_EINVAL, "sf_walk: connectivity %d (0 or 4: the agents' moves, 8)", p->connectivity);
    SF_TRY(check_points(who, p->k, p->points, true));
    if ((out->point_moves || out->point_step) && p->k == 0) return fail(SF_EINVAL, "sf_walk: point_moves and point_step need k > 0");
    if (out->point_step && p->connectivity == 8) return fail(SF_EINVAL, "sf_walk: point_step needs connectivity 4 (the four moves)");
    if (p->max_moves < 0) return fail(SF_EINVAL, "sf_walk: max_moves %d (0: no cap)", p->max_moves);
    SF_TRY(check_reserved(who, p->reserved[0] | p->reserved[1]));
    if (!out->moves && !out->point_moves && !out->point_step && !out->reached && !out->levels)
        return fail(SF_EINVAL, "sf_walk: every output is null");
    SF_TRY(check_aligned(who, ((uintptr_t)out->moves | (uintptr_t)out->point_moves | (uintptr_t)out->point_step | (uintptr_t)out->reached | (uintptr_t)out->levels) & 3));
    const size_t need = (size_t)walk_env_bytes(g);
    SF_TRY(check_scratch(who, p->scratch_bytes, need, "need"));
    SF_TRY(check_envs(s, who, n, envs));
    if (g.W > kWalkMaxWidth) return fail(SF_ENOTSUP, "sf_walk: grids wider than %d cells are not supported (width %d)", kWalkMaxWidth, g.W);
    SF_TRY(begin_call(s, who, kNeedRt | kNeedReset | kNotVoid));
    if (n == 0) return SF_OK;

    WalkArgs a;
    memset(&a, 0, sizeof a);
    band_args(s, a.band, p->passable, p->passable_per_env, p->k, p->target_mask, p->through_mask, p->connectivity == 8);
    a.targets = p->targets;
    a.tgt_env = p->targets_per_env ? (long long)g.H * g.W : 0;
    a.tgt_vec = p->targets && g.W % 16 == 0 && !((uintptr_t)p->targets & 15);
    a.max_moves = p->max_moves;
    a.moves_vec = out->moves && g.W % 4 == 0 && !((uintptr_t)out->moves & 15);
    const auto at = [&](int c0) {
        a.moves = out->moves ? out->moves + (size_t)c0 * g.H * g.W : nullptr;
        a.point_moves = out->point_moves ? out->point_moves + (size_t)c0 * p->k : nullptr;
        a.point_step = out->point_step ? out->point_step + (size_t)c0 * p->k : nullptr;
        a.reached = out->reached ? out->reached + c0 : nullptr;
        a.levels = out->levels ? out->levels + c0 : nullptr;
    };
    // (every point has a lane of its own, so a small grid still gets k threads)
    return band_search(s, who, s->walk, n, envs, p->points, p->scratch_bytes, kWalkScratchDefault, need, a, at, k_walk<true>, k_walk<false>,
                       std::max(a.band.nb, p->k), walk_lds_bytes);
}

// ----------------------------------------------------------------------------- escape routes
// A band search like sf_walk: one launch of k_escape per chunk, one workgroup per listed environment; the scratch of an environment
// holds the bit planes and halos, the cells sorted by deadline and the bounds of the buckets (escape_env_bytes).
extern "C" int sf_escape(sf_sim *s, const sf_escape_params *p, int32_t n, const int32_t *envs, const sf_escape_out *out)
{
    const char *who = "sf_escape";
    if (!s || !p || !out) return fail(SF_EINVAL, "sf_escape: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && !envs)) return fail(SF_EINVAL, "sf_escape: bad environment list");
    if (p->target_mask < 0 || p->target_mask > 63) return fail(SF_EINVAL, "sf_escape: target_mask %d (bit s selects BurnStatus s: 0..63)", p->target_mask);
    if (p->through_mask < 1 || p->through_mask > 63) return fail(SF_EINVAL, "sf_escape: through_mask %d (bit s selects BurnStatus s: 1..63)", p->through_mask);
    if (p->target_mask == 0 && !p->targets) return fail(SF_EINVAL, "sf_escape: target_mask 0 needs a targets plane");
    if (p->connectivity != 0 && p->connectivity != 4 && p->connectivity != 8)
        return fail(SF_EINVAL, "sf_escape: connectivity %d (0 or 4: the agents' moves, 8)", p->connectivity);
    if (p->flags & ~SF_ESCAPE_UNREACHED_SAFE) return fail(SF_EINVAL, "sf_escape: flags %d (0 or SF_ESCAPE_UNREACHED_SAFE)", p->flags);
    SF_TRY(check_points(who, p->k, p->points, true));
    if ((out->point_slack || out->point_step) && p->k == 0) return fail(SF_EINVAL, "sf_escape: point_slack and point_step need k > 0");
    if (!out->slack && !out->point_slack && !out->point_step && !out->safe && !out->escapable && !out->lost && !out->top)
        return fail(SF_EINVAL, "sf_escape: every output is null");
    SF_TRY(check_aligned(who, ((uintptr_t)out->slack | (uintptr_t)out->point_slack | (uintptr_t)out->point_step | (uintptr_t)out->safe | (uintptr_t)out->escapable |
                               (uintptr_t)out->lost | (uintptr_t)out->top | (uintptr_t)p->points | (uintptr_t)p->minutes) & 3));
    if (!std::isfinite(p->minutes_per_move) || !(p->minutes_per_move > 0.0)) return fail(SF_EINVAL, "sf_escape: minutes_per_move must be finite and > 0");
    if (!std::isfinite(p->margin_minutes) || !(p->margin_minutes >= 0.0)) return fail(SF_EINVAL, "sf_escape: margin_minutes must be finite and >= 0");
    if (!std::isfinite(p->horizon_minutes) || !(p->horizon_minutes > 0.0)) return fail(SF_EINVAL, "sf_escape: horizon_minutes must be finite and > 0");
    const double bound = std::ceil((p->horizon_minutes - p->margin_minutes) / p->minutes_per_move);      // (the kernel divides the same way: no deadline exceeds it)
    if (bound > (double)SF_ESCAPE_MAX_MOVES)
        return fail(SF_EINVAL, "sf_escape: the horizon is %.0f moves away, more than SF_ESCAPE_MAX_MOVES (%d)", bound, SF_ESCAPE_MAX_MOVES);
    if (!p->minutes) return fail(SF_EINVAL, "sf_escape: minutes is null");
    SF_TRY(check_reserved(who, p->reserved[0] | p->reserved[1]));
    const size_t need = (size_t)escape_env_bytes(g);
    SF_TRY(check_scratch(who, p->scratch_bytes, need, "need"));
    SF_TRY(check_envs(s, who, n, envs));
    if (g.W > kEscapeMaxWidth) return fail(SF_ENOTSUP, "sf_escape: grids wider than %d cells are not supported (width %d)", kEscapeMaxWidth, g.W);
    if ((long long)g.H * g.W >= (1ll << 31)) return fail(SF_ENOTSUP, "sf_escape: the cells of a %d x %d grid do not fit int32", g.H, g.W);
    SF_TRY(begin_call(s, who, kNeedRt | kNeedReset | kNotVoid));
    if (n == 0) return SF_OK;

    EscapeArgs a;
    memset(&a, 0, sizeof a);
    band_args(s, a.band, p->passable, p->passable_per_env, p->k, p->target_mask, p->through_mask, p->connectivity == 8);
    a.targets = p->targets;
    a.tgt_env = p->targets_per_env ? (long long)g.H * g.W : 0;
    a.tgt_vec = p->targets && g.W % 16 == 0 && !((uintptr_t)p->targets & 15);
    a.per_move = p->minutes_per_move; a.margin = p->margin_minutes; a.horizon = p->horizon_minutes;
    a.unreached_safe = (p->flags & SF_ESCAPE_UNREACHED_SAFE) != 0;
    a.bins = bound > 0.0 ? (int)bound : 0;
    a.slack_vec = out->slack && g.W % 4 == 0 && !((uintptr_t)out->slack & 15);
    a.o_list = escape_list_offset(g);
    a.o_buckets = (long long)need - kEscapeBoundsBytes;
    const auto at = [&](int c0) {
        a.minutes = p->minutes + (size_t)c0 * g.H * g.W;
        a.slack = out->slack ? out->slack + (size_t)c0 * g.H * g.W : nullptr;
        a.point_slack = out->point_slack ? out->point_slack + (size_t)c0 * p->k : nullptr;
        a.point_step = out->point_step ? out->point_step + (size_t)c0 * p->k : nullptr;
        a.safe = out->safe ? out->safe + c0 : nullptr;
        a.escapable = out->escapable ? out->escapable + c0 : nullptr;
        a.lost = out->lost ? out->lost + c0 : nullptr;
        a.top = out->top ? out->top + c0 : nullptr;
    };
    return band_search(s, who, s->escape, n, envs, p->points, p->scratch_bytes, kEscapeScratchDefault, need, a, at, k_escape<true>, k_escape<false>,
                       std::max(a.band.nb, p->k), escape_lds_bytes);
}

// ----------------------------------------------------------------------------- fire travel time
// One launch of k_travel per chunk, one workgroup per listed environment.  The working array of an environment is its row of the
// minutes plane where that is asked for (no scratch, no chunks but the launch grid's); else 4 * H * W bytes of scratch, as many
// environments per chunk as the budget holds.  The call block is the environment list; the arguments travel with the launch.
extern "C" int sf_travel(sf_sim *s, const sf_travel_params *p, int32_t n, const int32_t *envs, const sf_travel_out *out)
{
    const char *who = "sf_travel";
    if (!s || !p || !out) return fail(SF_EINVAL, "sf_travel: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && !envs)) return fail(SF_EINVAL, "sf_travel: bad environment list");
    if (p->source_mask < 0 || p->source_mask > 63) return fail(SF_EINVAL, "sf_travel: source_mask %d (bit s selects BurnStatus s: 0..63)", p->source_mask);
    if (p->through_mask < 1 || p->through_mask > 63) return fail(SF_EINVAL, "sf_travel: through_mask %d (bit s selects BurnStatus s: 1..63)", p->through_mask);
    if (p->source_mask == 0 && !p->sources) return fail(SF_EINVAL, "sf_travel: source_mask 0 needs a sources plane");
    if (p->connectivity != 0 && p->connectivity != 4 && p->connectivity != 8)
        return fail(SF_EINVAL, "sf_travel: connectivity %d (0: the handle's diagonal_spread, 4, 8)", p->connectivity);
    SF_TRY(check_points(who, p->k, p->points, true));
    if (out->point_minutes && p->k == 0) return fail(SF_EINVAL, "sf_travel: point_minutes needs k > 0");
    if (p->k > 0 && !out->point_minutes) return fail(SF_EINVAL, "sf_travel: points without point_minutes");
    if (!(p->max_minutes >= 0.0f)) return fail(SF_EINVAL, "sf_travel: max_minutes %g (0: no cap, or > 0)", (double)p->max_minutes);
    SF_TRY(check_reserved(who, p->reserved[0] | p->reserved[1]));
    if (!out->minutes && !out->pred && !out->point_minutes && !out->reached && !out->last && !out->activations)
        return fail(SF_EINVAL, "sf_travel: every output is null");
    SF_TRY(check_aligned(who, ((uintptr_t)out->minutes | (uintptr_t)out->point_minutes | (uintptr_t)out->reached | (uintptr_t)out->last |
                               (uintptr_t)out->activations | (uintptr_t)p->points) & 3));
    const size_t need = (size_t)travel_env_bytes(g);
    SF_TRY(check_scratch(who, p->scratch_bytes, need, "need"));
    SF_TRY(check_envs(s, who, n, envs));
    if (g.W > kTravelMaxWidth) return fail(SF_ENOTSUP, "sf_travel: grids wider than %d cells are not supported (width %d)", kTravelMaxWidth, g.W);
    const long long tiles = (long long)((g.W + kTravelTile - 1) / kTravelTile) * ((g.H + kTravelTile - 1) / kTravelTile);
    if (tiles > kTravelMaxTiles) return fail(SF_ENOTSUP, "sf_travel: a %d x %d grid has more than %d tiles", g.H, g.W, kTravelMaxTiles);
    SF_TRY(begin_call(s, who, kNeedRt | kNeedReset | kNotVoid));
    if (n == 0) return SF_OK;

    QueryState &q = s->travel;
    const size_t cells = (size_t)g.H * g.W;
    int chunk = std::min(n, 65535);
    if (!out->minutes) {
        chunk = query_chunk(n, p->scratch_bytes, kTravelScratchDefault, need, 65535);
        SF_TRY(scratch_reserve(s, q, (size_t)chunk * need));
    }
    const int32_t *envs_dev = nullptr;
    SF_TRY(block_stage(s, q.blk, &envs_dev, envs, (size_t)n * sizeof(int32_t)));

    TravelArgs a;
    memset(&a, 0, sizeof a);
    a.g = g;
    a.pl = cur_planes(s);
    a.rt = s->rt;
    a.sources = p->sources;
    a.src_env = p->sources_per_env ? (long long)cells : 0;
    a.passable = p->passable;
    a.pass_env = p->passable_per_env ? (long long)cells : 0;
    a.k = p->k;
    a.smask = (uint32_t)p->source_mask;
    a.tmask = (uint32_t)p->through_mask;
    a.conn8 = p->connectivity == 0 ? g.diag : (p->connectivity == 8);
    a.cap = p->max_minutes > 0.0f ? p->max_minutes : HUGE_VALF;
    a.work_env = out->minutes ? (long long)cells : (long long)(need / sizeof(float));
    a.fix_cap = out->minutes && p->max_minutes > 0.0f;
    a.pred_vec = out->pred && g.W % 4 == 0 && !((uintptr_t)out->pred & 3);
    const size_t lds = (size_t)((tiles + 31) / 32) * 2 * sizeof(uint32_t);
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int cn = std::min(chunk, n - c0);
        a.envs = envs_dev + c0;
        a.points = p->k ? p->points + (size_t)c0 * p->k * 3 : nullptr;
        a.work = out->minutes ? out->minutes + (size_t)c0 * cells : reinterpret_cast<float *>(q.mem);
        a.work_vec = g.W % 4 == 0 && !((uintptr_t)a.work & 15);
        a.pred = out->pred ? out->pred + (size_t)c0 * cells : nullptr;
        a.point_minutes = out->point_minutes ? out->point_minutes + (size_t)c0 * p->k : nullptr;
        a.reached = out->reached ? out->reached + c0 : nullptr;
        a.last = out->last ? out->last + c0 : nullptr;
        a.activations = out->activations ? out->activations + c0 : nullptr;
        hipLaunchKernelGGL(k_travel, dim3((unsigned)cn), dim3(kTravelThreads), lds, s->stream, a);
    }
    return finish_call(s, who, !s->async, nullptr);
}

// ----------------------------------------------------------------------------- fire behaviour
// The heat cache made current for the listed tables (host list), modelled on ensure_wterms: allocated at the first call, filled per
// run of stale tables.  Enqueue layer.
static int ensure_hpa(sf_sim *s, const std::vector<int32_t> &tabs)
{
    const Geo &g = s->g;
    BehaviorState &b = s->behavior;
    if (!b.hpa) {
        SF_TRY(dev_alloc(s, &b.hpa, (size_t)s->tables.size() * g.H * g.W));
        s->tables.hpa_allocated();
    }
    std::vector<int32_t> stale;
    for (int32_t t : tabs) if (s->tables[t].hpa_stale) stale.push_back(t);
    std::sort(stale.begin(), stale.end());
    stale.erase(std::unique(stale.begin(), stale.end()), stale.end());
    for (size_t i = 0; i < stale.size();) {
        size_t j = i + 1;
        while (j < stale.size() && stale[j] == stale[j - 1] + 1 && j - i < 65535) ++j;
        hipLaunchKernelGGL(k_behavior_hpa, dim3((unsigned)((g.W + kBehThreads - 1) / kBehThreads), (unsigned)g.H, (unsigned)(j - i)), dim3(kBehThreads), 0,
                           s->stream, g.H, g.W, (const double *)s->lay_all, (int)stale[i], (float)s->p.h, (float)s->p.S_T, (float)s->p.S_e,
                           (float)s->p.p_p, (float)s->p.M_f, b.hpa);
        for (size_t k = i; k < j; ++k) s->tables.hpa_built(stale[k]);
        b.builds += (int64_t)(j - i);
        i = j;
    }
    HIPCHK(hipGetLastError());
    return SF_OK;
}

// No scratch and no chunks: the stale parts of the heat cache are rebuilt, the summary outputs zeroed, then ONE launch serves the
// whole list: k_behavior where a plane is asked for, else k_behavior_scan.  No state of the handle changes but the cache.
extern "C" int sf_behavior(sf_sim *s, const sf_behavior_params *p, const sf_behavior_out *out, const int32_t *envs, int32_t n)
{
    const char *who = "sf_behavior";
    if (!s || !p || !out) return fail(SF_EINVAL, "sf_behavior: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && !envs)) return fail(SF_EINVAL, "sf_behavior: bad environment list");
    const bool planes = out->hpa || out->ros || out->intensity || out->flame_length || out->head || out->workable;
    const bool summary = out->max_flame || out->max_intensity || out->classes;
    if (!planes && !summary && !out->point_flame) return fail(SF_EINVAL, "sf_behavior: every output is null");
    if (p->status_mask < 0 || p->status_mask > 63) return fail(SF_EINVAL, "sf_behavior: status_mask %d (bit s selects BurnStatus s: 1..63, or 0 for every cell)", p->status_mask);
    if (p->summary_mask < 1 || p->summary_mask > 63) return fail(SF_EINVAL, "sf_behavior: summary_mask %d (bit s selects BurnStatus s: 1..63)", p->summary_mask);
    SF_TRY(check_reserved(who, p->reserved));
    if (!(p->edges[0] < p->edges[1] && p->edges[1] < p->edges[2] && p->edges[2] < p->edges[3]))
        return fail(SF_EINVAL, "sf_behavior: the class edges must increase (%g, %g, %g, %g)", (double)p->edges[0], (double)p->edges[1], (double)p->edges[2], (double)p->edges[3]);
    if (!(p->flame_limit >= 0.0f)) return fail(SF_EINVAL, "sf_behavior: flame_limit %g (>= 0)", (double)p->flame_limit);
    SF_TRY(check_points(who, p->k, p->points, true));
    if (out->point_flame && p->k == 0) return fail(SF_EINVAL, "sf_behavior: point_flame needs k > 0");
    if (p->k > 0 && !out->point_flame) return fail(SF_EINVAL, "sf_behavior: points without point_flame");
    SF_TRY(check_aligned(who, ((uintptr_t)out->hpa | (uintptr_t)out->ros | (uintptr_t)out->intensity | (uintptr_t)out->flame_length | (uintptr_t)out->max_flame |
                               (uintptr_t)out->max_intensity | (uintptr_t)out->classes | (uintptr_t)out->point_flame | (uintptr_t)p->points) & 3));
    SF_TRY(check_envs(s, who, n, envs));
    SF_TRY(check_ready(s, who, kNeedRt | kNeedReset));
    const bool per_env = s->tables.size() > 1;
    std::vector<int32_t> tabs;
    for (int i = 0; i < n; ++i) {
        const int t = per_env ? envs[i] : 0;
        if (!s->tables[t].layers)
            return fail(SF_ESTATE, "sf_behavior: environment %d's table came from sf_set_rtable: there are no layers to take the reaction intensity from", envs[i]);
        tabs.push_back(t);
    }
    SF_TRY(begin_call(s, who, kNeedRt | kNeedReset | kNotVoid));
    if (n == 0) return SF_OK;

    BehaviorState &b = s->behavior;
    SF_TRY(ensure_hpa(s, tabs));
    BehArgs a;
    memset(&a, 0, sizeof a);
    SF_TRY(block_stage(s, b.blk, &a.envs, envs, (size_t)n * sizeof(int32_t)));
    if (out->max_flame) HIPCHK(hipMemsetAsync(out->max_flame, 0, (size_t)n * sizeof(float), s->stream));
    if (out->max_intensity) HIPCHK(hipMemsetAsync(out->max_intensity, 0, (size_t)n * sizeof(float), s->stream));
    if (out->classes) HIPCHK(hipMemsetAsync(out->classes, 0, (size_t)n * 5 * sizeof(int32_t), s->stream));

    a.g = cell_geo(g);
    a.pl = cur_planes(s);
    a.rt_env = g.rt_env;
    a.rt = s->rt;
    a.hpa = b.hpa;
    a.hpa_env = per_env ? (long long)g.H * g.W : 0;
    a.n = n;
    a.smask = (uint32_t)p->status_mask;
    a.summask = (uint32_t)p->summary_mask;
    a.flame_limit = p->flame_limit;
    for (int i = 0; i < 4; ++i) a.edge[i] = p->edges[i];
    a.o_hpa = out->hpa; a.o_ros = out->ros; a.o_int = out->intensity; a.o_flame = out->flame_length; a.o_head = out->head; a.o_work = out->workable;
    a.max_flame = out->max_flame; a.max_int = out->max_intensity; a.classes = out->classes;
    a.points = p->points; a.point_flame = out->point_flame; a.k = p->k;
    a.planes = planes; a.summary = summary;
    // items per environment: (row, 4 columns) with planes, (row, 16-cell vector) for the scan
    a.blocks_env = ((long long)g.H * (planes ? (g.W + 3) / 4 : g.PV) + kBehThreads - 1) / kBehThreads;
    a.total = (planes || summary) ? (long long)n * a.blocks_env : 0;
    const bool vec = g.W % 4 == 0 && !(((uintptr_t)out->hpa | (uintptr_t)out->ros | (uintptr_t)out->intensity | (uintptr_t)out->flame_length) & 15) &&
                     !(((uintptr_t)out->head | (uintptr_t)out->workable) & 3);
    const long long pblocks = ((long long)n * p->k + kBehThreads - 1) / kBehThreads;
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(std::max(a.total, pblocks), (long long)s->n_cu * 8));
    if (!planes) hipLaunchKernelGGL(k_behavior_scan, dim3(grid), dim3(kBehThreads), 0, s->stream, a);
    else if (vec) hipLaunchKernelGGL(k_behavior<true>, dim3(grid), dim3(kBehThreads), 0, s->stream, a);
    else hipLaunchKernelGGL(k_behavior<false>, dim3(grid), dim3(kBehThreads), 0, s->stream, a);
    return finish_call(s, who, !s->async, nullptr);
}

extern "C" int sf_get_behavior_builds(sf_sim *s, int64_t *n_out)
{
    if (!s || !n_out) return fail(SF_EINVAL, "sf_get_behavior_builds: null argument");
    *n_out = s->behavior.builds;
    return SF_OK;
}

// ----------------------------------------------------------------------------- perimeters of the fire
// Without a traced output: the summary outputs zeroed, then ONE launch of k_perim_summary for the whole list - no scratch, no chunks.
// With one: k_perim_trace, one workgroup per listed environment, chunk by chunk as the scratch budget allows (it writes edges and
// cells itself); a front plane asked for beside it comes from a launch of k_perim_summary.  The call block is the environment list.
extern "C" int sf_perimeter(sf_sim *s, const sf_perimeter_params *p, int32_t n, const int32_t *envs, const sf_perimeter_out *out)
{
    const char *who = "sf_perimeter";
    if (!s || !p || !out) return fail(SF_EINVAL, "sf_perimeter: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && !envs)) return fail(SF_EINVAL, "sf_perimeter: bad environment list");
    if (p->status_mask < 0 || p->status_mask > 63) return fail(SF_EINVAL, "sf_perimeter: status_mask %d (bit s selects BurnStatus s: 1..63, or 0 with member or at_update)", p->status_mask);
    if (p->at_update < -1) return fail(SF_EINVAL, "sf_perimeter: at_update %d (-1: off, or an update >= 0)", p->at_update);
    const int sources = (p->status_mask != 0) + (p->member != nullptr) + (p->at_update >= 0);
    if (sources != 1) return fail(SF_EINVAL, "sf_perimeter: %s (exactly one of status_mask, member, at_update)", sources ? "more than one source" : "no source");
    if (p->connectivity != 0 && p->connectivity != 4 && p->connectivity != 8)
        return fail(SF_EINVAL, "sf_perimeter: connectivity %d (0: the handle's diagonal_spread, 4, 8)", p->connectivity);
    if (p->max_edges < 0 || p->max_vertices < 0 || p->max_loops < 0)
        return fail(SF_EINVAL, "sf_perimeter: negative capacity (max_edges %d, max_vertices %d, max_loops %d)", p->max_edges, p->max_vertices, p->max_loops);
    if (out->vertices && p->max_vertices == 0) return fail(SF_EINVAL, "sf_perimeter: vertices needs max_vertices > 0");
    if ((out->loop_start || out->loop_area || out->loop_edges) && p->max_loops == 0)
        return fail(SF_EINVAL, "sf_perimeter: loop_start, loop_area and loop_edges need max_loops > 0");
    const bool traced = out->loops || out->holes || out->n_vertices || out->vertices || out->loop_start || out->loop_area || out->loop_edges;
    if (!traced && !out->edges && !out->cells && !out->front) return fail(SF_EINVAL, "sf_perimeter: every output is null");
    SF_TRY(check_aligned(who, ((uintptr_t)out->edges | (uintptr_t)out->cells | (uintptr_t)out->loops | (uintptr_t)out->holes | (uintptr_t)out->n_vertices |
                               (uintptr_t)out->vertices | (uintptr_t)out->loop_start | (uintptr_t)out->loop_area | (uintptr_t)out->loop_edges) & 3));
    const size_t need = traced ? (size_t)perim_env_bytes(g.H, g.W, p->max_edges) : 0;
    SF_TRY(check_scratch(who, p->scratch_bytes, need, "need"));
    SF_TRY(check_reserved(who, p->reserved[0] | p->reserved[1]));
    SF_TRY(check_envs(s, who, n, envs));
    if (g.W > kPerimMaxWidth) return fail(SF_ENOTSUP, "sf_perimeter: grids wider than %d cells are not supported (width %d)", kPerimMaxWidth, g.W);
    if ((long long)(g.H + 1) * ((g.W + 16) / 16) >= (1ll << 25)) return fail(SF_ENOTSUP, "sf_perimeter: the edge ids of a %d x %d grid do not fit int32", g.H, g.W);
    SF_TRY(check_ready(s, who, kNeedReset));
    if (p->at_update >= 0 && !s->arrival.plane) return fail(SF_ESTATE, "sf_perimeter: at_update needs arrival recording (sf_enable_arrival)");
    SF_TRY(begin_call(s, who, kNeedReset | kNotVoid));
    if (n == 0) return SF_OK;

    QueryState &q = s->perimeter;
    PerimArgs a;
    memset(&a, 0, sizeof a);
    const size_t cells = (size_t)g.H * g.W;
    int chunk = n;
    if (traced) {
        chunk = query_chunk(n, p->scratch_bytes, kPerimScratchDefault, need, 65535);
        SF_TRY(scratch_reserve(s, q, (size_t)chunk * need));
    }
    const int32_t *envs_dev = nullptr;
    SF_TRY(block_stage(s, q.blk, &envs_dev, envs, (size_t)n * sizeof(int32_t)));
    a.g = cell_geo(g);
    a.pl = cur_planes(s);
    a.member = p->member;
    a.mem_env = p->member_per_env ? (long long)cells : 0;
    a.arrival = s->arrival.plane;
    a.at = (uint32_t)std::max(p->at_update, 0);
    a.source = p->member ? 1 : (p->at_update >= 0 ? 2 : 0);
    mask_tables(p->status_mask, a.tlo, a.thi);
    a.conn8 = p->connectivity == 0 ? g.diag : (p->connectivity == 8);
    a.simplify = p->simplify != 0;
    a.max_edges = p->max_edges; a.max_vertices = p->max_vertices; a.max_loops = p->max_loops;
    a.BW = (g.W + 63) / 64; a.EW = (g.W + 16) / 16;
    a.blocks_env = ((long long)((g.H + kPerimStrip - 1) / kPerimStrip) * a.BW + kPerimThreads - 1) / kPerimThreads;

    if (!traced || out->front) {                 // the summary form, or the front plane of a traced call
        PerimArgs b = a;
        b.envs = envs_dev;
        b.n = n;
        b.total = (long long)n * b.blocks_env;
        b.front = out->front;
        b.front_vec = out->front && g.W % 16 == 0 && !((uintptr_t)out->front & 15);
        if (!traced) {
            b.edges = out->edges; b.ncells = out->cells;
            if (out->edges) HIPCHK(hipMemsetAsync(out->edges, 0, (size_t)n * sizeof(int32_t), s->stream));
            if (out->cells) HIPCHK(hipMemsetAsync(out->cells, 0, (size_t)n * sizeof(int32_t), s->stream));
        }
        const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(b.total, (long long)s->n_cu * 8));
        hipLaunchKernelGGL(k_perim_summary, dim3(grid), dim3(kPerimThreads), 0, s->stream, b);
    }
    if (traced) {
        a.scratch = q.mem;
        a.scratch_env = (long long)need;
        for (int c0 = 0; c0 < n; c0 += chunk) {
            a.n = std::min(chunk, n - c0);
            a.envs = envs_dev + c0;
            a.edges = out->edges ? out->edges + c0 : nullptr;
            a.ncells = out->cells ? out->cells + c0 : nullptr;
            a.loops = out->loops ? out->loops + c0 : nullptr;
            a.holes = out->holes ? out->holes + c0 : nullptr;
            a.n_vertices = out->n_vertices ? out->n_vertices + c0 : nullptr;
            a.vertices = out->vertices ? out->vertices + (size_t)c0 * p->max_vertices * 2 : nullptr;
            a.loop_start = out->loop_start ? out->loop_start + (size_t)c0 * ((size_t)p->max_loops + 1) : nullptr;
            a.loop_area = out->loop_area ? out->loop_area + (size_t)c0 * p->max_loops : nullptr;
            a.loop_edges = out->loop_edges ? out->loop_edges + (size_t)c0 * p->max_loops : nullptr;
            hipLaunchKernelGGL(k_perim_trace, dim3((unsigned)a.n), dim3(kPerimTraceThreads), 0, s->stream, a);
        }
    }
    return finish_call(s, who, !s->async, nullptr);
}

// ----------------------------------------------------------------------------- fire influence
// Per chunk: the counters zeroed, then k_infl_stage, k_infl_walk, k_infl_finish and - with points - k_infl_points, a thread per cell
// (per point).  The scratch of a listed environment holds the sanitised codes, the child counters and whichever accumulator is no
// output of the call (infl_env_bytes).  The call block is the environment list; the arguments travel with the launches.
extern "C" int sf_influence(sf_sim *s, const sf_influence_params *p, int32_t n, const int32_t *envs, const sf_influence_out *out)
{
    const char *who = "sf_influence";
    if (!s || !p || !out) return fail(SF_EINVAL, "sf_influence: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && !envs)) return fail(SF_EINVAL, "sf_influence: bad environment list");
    if (p->pred_source != SF_INFLUENCE_PRED_PLANE && p->pred_source != SF_INFLUENCE_PRED_HISTORY)
        return fail(SF_EINVAL, "sf_influence: pred_source %d (0: a pred plane, 1: the episode's history)", p->pred_source);
    if (p->weight_mode < SF_INFLUENCE_WEIGHT_NONE || p->weight_mode > SF_INFLUENCE_WEIGHT_PLANE)
        return fail(SF_EINVAL, "sf_influence: weight_mode %d (0: none, 1: the handle's value plane, 2: a weights plane)", p->weight_mode);
    const bool history = p->pred_source == SF_INFLUENCE_PRED_HISTORY;
    if (!history && !p->pred) return fail(SF_EINVAL, "sf_influence: pred_source 0 needs a pred plane");
    if (history && p->pred) return fail(SF_EINVAL, "sf_influence: pred_source 1 (history) takes no pred plane");
    if ((p->weight_mode == SF_INFLUENCE_WEIGHT_PLANE) != (p->weights != nullptr))
        return fail(SF_EINVAL, "sf_influence: weight_mode 2 and a weights plane go together");
    const bool weighted = p->weight_mode != SF_INFLUENCE_WEIGHT_NONE;
    if ((out->value || out->point_value) && !weighted) return fail(SF_EINVAL, "sf_influence: value and point_value need weights (weight_mode 1 or 2)");
    SF_TRY(check_points(who, p->k, p->points, true));
    if (p->max_route < 0 || p->max_route > kInflMaxRoute) return fail(SF_EINVAL, "sf_influence: max_route %d (0: no routes, at most %d)", p->max_route, kInflMaxRoute);
    const bool point_out = out->point_cells || out->point_value || out->point_route || out->point_hops;
    if (point_out && p->k == 0) return fail(SF_EINVAL, "sf_influence: point outputs need k > 0");
    if (p->k > 0 && !point_out) return fail(SF_EINVAL, "sf_influence: points without a point output");
    if (p->max_route > 0 && (!out->point_route || !out->point_hops)) return fail(SF_EINVAL, "sf_influence: max_route > 0 needs point_route and point_hops");
    if (p->max_route == 0 && (out->point_route || out->point_hops)) return fail(SF_EINVAL, "sf_influence: point_route and point_hops need max_route > 0");
    SF_TRY(check_aligned(who, (((uintptr_t)out->cells | (uintptr_t)out->forest | (uintptr_t)out->roots | (uintptr_t)out->cyclic | (uintptr_t)out->point_cells |
                                (uintptr_t)out->point_route | (uintptr_t)out->point_hops | (uintptr_t)p->points | (uintptr_t)p->weights) & 3) |
                                   (((uintptr_t)out->value | (uintptr_t)out->point_value) & 7)));
    const size_t need = (size_t)infl_env_bytes(g.H, g.W, out->cells != nullptr, weighted, out->value != nullptr);
    SF_TRY(check_scratch(who, p->scratch_bytes, need, "need"));
    SF_TRY(check_reserved(who, p->reserved[0] | p->reserved[1]));
    if (!out->cells && !out->value && !out->pred && !out->forest && !out->roots && !out->cyclic && !point_out)
        return fail(SF_EINVAL, "sf_influence: every output is null");
    SF_TRY(check_envs(s, who, n, envs));
    if (g.W > kInflMaxWidth) return fail(SF_ENOTSUP, "sf_influence: grids wider than %d cells are not supported (width %d)", kInflMaxWidth, g.W);
    if ((long long)g.H * g.W >= (1ll << 31)) return fail(SF_ENOTSUP, "sf_influence: the cells of a %d x %d grid do not fit int32", g.H, g.W);
    SF_TRY(check_ready(s, who, kNeedReset));
    // (a graph switched off keeps its masks allocated, but they miss every ignition since: no tree from those)
    if (history && !(s->parents && s->graph_on)) return fail(SF_ESTATE, "sf_influence: the history source needs the spread graph (sf_enable_spread_graph)");
    if (history && !s->arrival.plane) return fail(SF_ESTATE, "sf_influence: the history source needs arrival recording (sf_enable_arrival)");
    if (p->weight_mode == SF_INFLUENCE_WEIGHT_VALUES && !s->values.plane) return fail(SF_ESTATE, "sf_influence: weight_mode 1 needs a value plane (sf_values_set)");
    SF_TRY(begin_call(s, who, kNeedReset | kNotVoid));
    if (n == 0) return SF_OK;

    QueryState &q = s->influence;
    const size_t cells = (size_t)g.H * g.W;
    const int chunk = query_chunk(n, p->scratch_bytes, kInflScratchDefault, need, 65535);      // (65535: the launch grid's y)
    SF_TRY(scratch_reserve(s, q, (size_t)chunk * need));
    const int32_t *envs_dev = nullptr;
    SF_TRY(block_stage(s, q.blk, &envs_dev, envs, (size_t)n * sizeof(int32_t)));
    for (int32_t *cnt : {out->forest, out->roots, out->cyclic})
        if (cnt) HIPCHK(hipMemsetAsync(cnt, 0, (size_t)n * sizeof(int32_t), s->stream));

    InflArgs a;
    memset(&a, 0, sizeof a);
    a.H = g.H; a.W = g.W; a.P = g.P;
    a.plane_env = g.plane_env;
    a.source = p->pred_source;
    a.pred_env = p->pred_per_env ? (long long)cells : 0;
    a.parents = s->parents;
    a.arrival = s->arrival.plane;
    a.include = p->include;
    a.inc_env = p->include_per_env ? (long long)cells : 0;
    if (p->weight_mode == SF_INFLUENCE_WEIGHT_VALUES) {
        a.weights = s->values.plane; a.w_env = s->values.per_env ? g.plane_env : 0; a.w_pitch = g.P;
    } else if (weighted) {
        a.weights = p->weights; a.w_env = p->weights_per_env ? (long long)cells : 0; a.w_pitch = g.W;
    }
    a.inclusive = p->inclusive != 0;
    a.scratch = q.mem;
    a.scratch_env = (long long)need;
    a.o_cnt = infl_round((long long)cells);
    long long o = a.o_cnt + infl_round(4 * (long long)cells);
    a.o_acc_c = -1; a.o_acc_v = -1;
    if (!out->cells) { a.o_acc_c = o; o += infl_round(4 * (long long)cells); }
    if (weighted && !out->value) { a.o_acc_v = o; o += infl_round(8 * (long long)cells); }
    a.k = p->k; a.max_route = p->max_route;
    const unsigned cell_blocks = (unsigned)((cells + kInflThreads - 1) / kInflThreads);
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int cn = std::min(chunk, n - c0);
        a.envs = envs_dev + c0;
        a.pred_in = p->pred ? p->pred + (size_t)c0 * (size_t)a.pred_env : nullptr;
        a.cells = out->cells ? out->cells + (size_t)c0 * cells : nullptr;
        a.value = out->value ? reinterpret_cast<long long *>(out->value) + (size_t)c0 * cells : nullptr;
        a.pred_out = out->pred ? out->pred + (size_t)c0 * cells : nullptr;
        a.forest = out->forest ? out->forest + c0 : nullptr;
        a.roots = out->roots ? out->roots + c0 : nullptr;
        a.cyclic = out->cyclic ? out->cyclic + c0 : nullptr;
        a.points = p->k ? p->points + (size_t)c0 * p->k * 3 : nullptr;
        a.point_cells = out->point_cells ? out->point_cells + (size_t)c0 * p->k : nullptr;
        a.point_value = out->point_value ? reinterpret_cast<long long *>(out->point_value) + (size_t)c0 * p->k : nullptr;
        a.point_route = out->point_route ? out->point_route + (size_t)c0 * p->k * p->max_route : nullptr;
        a.point_hops = out->point_hops ? out->point_hops + (size_t)c0 * p->k : nullptr;
        HIPCHK(hipMemset2DAsync(q.mem + a.o_cnt, need, 0, cells * sizeof(int32_t), (size_t)cn, s->stream));
        hipLaunchKernelGGL(k_infl_stage, dim3(cell_blocks, (unsigned)cn), dim3(kInflThreads), 0, s->stream, a);
        hipLaunchKernelGGL(k_infl_walk, dim3(cell_blocks, (unsigned)cn), dim3(kInflThreads), 0, s->stream, a);
        hipLaunchKernelGGL(k_infl_finish, dim3(cell_blocks, (unsigned)cn), dim3(kInflThreads), 0, s->stream, a);
        if (p->k)
            hipLaunchKernelGGL(k_infl_points, dim3((unsigned)(((long long)cn * p->k + kInflThreads - 1) / kInflThreads)), dim3(kInflThreads), 0, s->stream, a, cn);
    }
    return finish_call(s, who, !s->async, nullptr);
}

// ----------------------------------------------------------------------------- connected components
// Per chunk: the head of every environment's scratch zeroed, then k_comp_stage, k_comp_merge, k_comp_heads, k_comp_flatten and
// k_comp_scan (count is done here); with any output beyond count and selected k_comp_assign and k_comp_relabel; with a stats row or
// largest k_comp_stats (around it k_comp_zero and k_comp_largest); with largest or points k_comp_finish.  The scratch of a listed
// environment is cc_env_bytes: the label plane is the caller's labels output where that is asked for.  The call block is the
// environment list | one CompArgs per chunk; the kernels take their arguments from there.
extern "C" int sf_components(sf_sim *s, const sf_components_params *p, int32_t n, const int32_t *envs, const sf_components_out *out)
{
    const char *who = "sf_components";
    if (!s || !p || !out) return fail(SF_EINVAL, "sf_components: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && !envs)) return fail(SF_EINVAL, "sf_components: bad environment list");
    if (p->select_mask < 1 || p->select_mask > 63) return fail(SF_EINVAL, "sf_components: select_mask %d (bit s selects BurnStatus s: 1..63)", p->select_mask);
    if (p->connectivity != 0 && p->connectivity != 4 && p->connectivity != 8)
        return fail(SF_EINVAL, "sf_components: connectivity %d (0: the handle's diagonal_spread, 4, 8)", p->connectivity);
    SF_TRY(check_points(who, p->k, p->points, true));
    if (p->max_components < 1 || p->max_components > kCompMaxCap)
        return fail(SF_EINVAL, "sf_components: max_components %d (1..%d)", p->max_components, kCompMaxCap);
    if (out->point_label && p->k == 0) return fail(SF_EINVAL, "sf_components: point_label needs k > 0");
    if (p->k > 0 && !out->point_label) return fail(SF_EINVAL, "sf_components: points without point_label");
    SF_TRY(check_reserved(who, p->reserved0 | p->reserved[0] | p->reserved[1]));
    if (!out->count && !out->selected && !out->labels && !out->cells && !out->value && !out->first && !out->bbox && !out->touch && !out->largest && !out->point_label)
        return fail(SF_EINVAL, "sf_components: every output is null");
    SF_TRY(check_aligned(who, (((uintptr_t)out->count | (uintptr_t)out->selected | (uintptr_t)out->labels | (uintptr_t)out->cells | (uintptr_t)out->first |
                                (uintptr_t)out->bbox | (uintptr_t)out->touch | (uintptr_t)out->largest | (uintptr_t)out->point_label | (uintptr_t)p->points) & 3) |
                                   ((uintptr_t)out->value & 7)));
    const size_t need = (size_t)cc_env_bytes(g.H, g.W, out->labels != nullptr);
    SF_TRY(check_scratch(who, p->scratch_bytes, need, "need"));
    SF_TRY(check_envs(s, who, n, envs));
    if (out->value && !s->values.plane) return fail(SF_EINVAL, "sf_components: value needs a value plane (sf_values_set)");
    if (g.W > kCompMaxWidth) return fail(SF_ENOTSUP, "sf_components: grids wider than %d cells are not supported (width %d)", kCompMaxWidth, g.W);
    if ((long long)g.H * g.W >= (1ll << 31)) return fail(SF_ENOTSUP, "sf_components: the cells of a %d x %d grid do not fit int32", g.H, g.W);
    SF_TRY(begin_call(s, who, kNeedReset | kNotVoid));
    if (n == 0) return SF_OK;

    QueryState &q = s->components;
    const size_t cells = (size_t)g.H * g.W;
    const int cap = p->max_components;
    const int chunk = query_chunk(n, p->scratch_bytes, kCompScratchDefault, need, 65535), chunks = (n + chunk - 1) / chunk;      // (65535: the launch grid's y)
    SF_TRY(scratch_reserve(s, q, (size_t)chunk * need));
    SF_TRY(lab_start(s, s->components_timer));
    // rows past the count: 0 (cells, value, touch) and -1 (first, bbox); selected is added to
    if (out->selected) HIPCHK(hipMemsetAsync(out->selected, 0, (size_t)n * sizeof(int32_t), s->stream));
    if (out->cells) HIPCHK(hipMemsetAsync(out->cells, 0, (size_t)n * cap * sizeof(int32_t), s->stream));
    if (out->value) HIPCHK(hipMemsetAsync(out->value, 0, (size_t)n * cap * sizeof(int64_t), s->stream));
    if (out->touch) HIPCHK(hipMemsetAsync(out->touch, 0, (size_t)n * cap * sizeof(int32_t), s->stream));
    if (out->first) HIPCHK(hipMemsetAsync(out->first, 0xFF, (size_t)n * cap * sizeof(int32_t), s->stream));
    if (out->bbox) HIPCHK(hipMemsetAsync(out->bbox, 0xFF, (size_t)n * cap * 4 * sizeof(int32_t), s->stream));

    CompArgs a;
    memset(&a, 0, sizeof a);
    a.g = cell_geo(g);
    a.pl = cur_planes(s);
    a.member = p->member;
    a.mem_env = p->member_per_env ? (long long)cells : 0;
    a.mem_vec = p->member && g.W % 16 == 0 && !((uintptr_t)p->member & 15);
    mask_tables(p->select_mask, a.tlo, a.thi);
    a.conn8 = p->connectivity == 0 ? g.diag : (p->connectivity == 8);
    a.WORDS = cc_words(g.W);
    a.cap = cap;
    a.k = p->k;
    a.scratch = q.mem;
    a.scratch_env = (long long)need;
    a.o_rows = cc_off_rows(g.H, g.W); a.o_aux = cc_off_aux(g.H, g.W); a.o_par = cc_off_par(g.H, g.W);
    a.vals = out->value ? s->values.plane : nullptr;
    a.val_env = s->values.per_env ? g.plane_env : 0;
    a.lab_vec = cells % 4 == 0 && !((uintptr_t)out->labels & 15);

    const size_t o_args = ((size_t)n * sizeof(int32_t) + 15) / 16 * 16, bytes = o_args + (size_t)chunks * sizeof(CompArgs);
    SF_TRY(block_reserve(s, q.blk, bytes));
    memcpy(q.blk.pinned, envs, (size_t)n * sizeof(int32_t));
    for (int c = 0; c < chunks; ++c) {
        const int c0 = c * chunk;
        a.envs = reinterpret_cast<const int32_t *>(q.blk.dev) + c0;
        a.points = p->k ? p->points + (size_t)c0 * p->k * 3 : nullptr;
        a.count = out->count ? out->count + c0 : nullptr;
        a.selected = out->selected ? out->selected + c0 : nullptr;
        a.labels = out->labels ? out->labels + (size_t)c0 * cells : nullptr;
        a.cells = out->cells ? out->cells + (size_t)c0 * cap : nullptr;
        a.value = out->value ? reinterpret_cast<long long *>(out->value) + (size_t)c0 * cap : nullptr;
        a.first = out->first ? out->first + (size_t)c0 * cap : nullptr;
        a.bbox = out->bbox ? out->bbox + (size_t)c0 * cap * 4 : nullptr;
        a.touch = out->touch ? out->touch + (size_t)c0 * cap : nullptr;
        a.largest = out->largest ? out->largest + (size_t)c0 * 2 : nullptr;
        a.point_label = out->point_label ? out->point_label + (size_t)c0 * p->k : nullptr;
        memcpy(q.blk.pinned + o_args + (size_t)c * sizeof(CompArgs), &a, sizeof a);
    }
    SF_TRY(block_send(s, q.blk, bytes));

    const bool stats = out->cells || out->value || out->bbox || out->touch || out->largest;
    const bool numbered = stats || out->labels || out->first || out->point_label;
    const unsigned row_blocks = (unsigned)((g.H + kCompThreads / 64 - 1) / (kCompThreads / 64));
    const unsigned word_blocks = (unsigned)(((long long)g.H * a.WORDS + kCompThreads - 1) / kCompThreads);
    const unsigned cell_blocks = (unsigned)(((a.lab_vec ? cells / 4 : cells) + kCompThreads - 1) / kCompThreads);
    const unsigned max_blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((cells / 2 + kCompThreads * 8 - 1) / (kCompThreads * 8), 64));
    for (int c = 0; c < chunks; ++c) {
        const unsigned cn = (unsigned)std::min(chunk, n - c * chunk);
        const CompArgs *ap = reinterpret_cast<const CompArgs *>(q.blk.dev + o_args) + c;
        HIPCHK(hipMemset2DAsync(q.mem, need, 0, kCompHeadBytes, cn, s->stream));
        hipLaunchKernelGGL(k_comp_stage, dim3(row_blocks, cn), dim3(kCompThreads), 0, s->stream, ap);
        hipLaunchKernelGGL(k_comp_merge, dim3(word_blocks, cn), dim3(kCompThreads), 0, s->stream, ap);
        hipLaunchKernelGGL(k_comp_heads, dim3(word_blocks, cn), dim3(kCompThreads), 0, s->stream, ap);
        hipLaunchKernelGGL(k_comp_flatten, dim3(row_blocks, cn), dim3(kCompThreads), 0, s->stream, ap);
        hipLaunchKernelGGL(k_comp_scan, dim3(cn), dim3(kCompScanThreads), 0, s->stream, ap);
        if (!numbered) continue;
        hipLaunchKernelGGL(k_comp_assign, dim3(row_blocks, cn), dim3(kCompThreads), 0, s->stream, ap);
        hipLaunchKernelGGL(k_comp_relabel, dim3(cell_blocks, cn), dim3(kCompThreads), 0, s->stream, ap);
        if (stats) {
            if (out->largest) hipLaunchKernelGGL(k_comp_zero, dim3(max_blocks, cn), dim3(kCompThreads), 0, s->stream, ap);
            hipLaunchKernelGGL(k_comp_stats, dim3(word_blocks, cn), dim3(kCompThreads), 0, s->stream, ap);
            if (out->largest) hipLaunchKernelGGL(k_comp_largest, dim3(max_blocks, cn), dim3(kCompThreads), 0, s->stream, ap);
        }
        if (out->largest || p->k)
            hipLaunchKernelGGL(k_comp_finish, dim3((unsigned)(((long long)cn * (p->k + 1) + kCompThreads - 1) / kCompThreads)), dim3(kCompThreads), 0, s->stream, ap, (int)cn);
    }
    SF_TRY(lab_stop(s, s->components_timer));
    return finish_call(s, who, !s->async, nullptr);
}

extern "C" int sf_time_components(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_time_components: null handle");
    s->components_timer = {on != 0, false};
    return SF_OK;
}

extern "C" int sf_get_components_ms(sf_sim *s, float *ms_out)
{
    if (!s || !ms_out) return fail(SF_EINVAL, "sf_get_components_ms: null argument");
    return lab_ms(s, s->components_timer, "sf_get_components_ms", "no sf_components call has been timed (sf_time_components)", ms_out);
}
