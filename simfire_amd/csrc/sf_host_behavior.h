// Host code of sf_behavior: fireline intensity and flame length per cell.  Included once from simfire_hip.hip,
// behind sf_host_walk.h (whose sf_walk it follows point by point in what a call may and may not do).
#pragma once

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

// The environment list goes through the feature's call block; the summary outputs are zeroed, the stale parts of the heat cache
// rebuilt, then ONE launch serves the whole list: k_behavior where a plane is asked for, else k_behavior_scan.  All of it on the handle's stream; no state of the handle changes but
// the cache.
extern "C" int sf_behavior(sf_sim *s, const sf_behavior_params *p, const sf_behavior_out *out, const int32_t *envs, int32_t n)
{
    if (!s || !p || !out) return fail(SF_EINVAL, "sf_behavior: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && !envs)) return fail(SF_EINVAL, "sf_behavior: bad environment list");
    const bool planes = out->hpa || out->ros || out->intensity || out->flame_length || out->head || out->workable;
    const bool summary = out->max_flame || out->max_intensity || out->classes;
    if (!planes && !summary && !out->point_flame) return fail(SF_EINVAL, "sf_behavior: every output is null");
    if (p->status_mask < 0 || p->status_mask > 63) return fail(SF_EINVAL, "sf_behavior: status_mask %d (bit s selects BurnStatus s: 1..63, or 0 for every cell)", p->status_mask);
    if (p->summary_mask < 1 || p->summary_mask > 63) return fail(SF_EINVAL, "sf_behavior: summary_mask %d (bit s selects BurnStatus s: 1..63)", p->summary_mask);
    if (p->reserved != 0) return fail(SF_EINVAL, "sf_behavior: reserved must be 0");
    if (!(p->edges[0] < p->edges[1] && p->edges[1] < p->edges[2] && p->edges[2] < p->edges[3]))
        return fail(SF_EINVAL, "sf_behavior: the class edges must increase (%g, %g, %g, %g)", (double)p->edges[0], (double)p->edges[1], (double)p->edges[2], (double)p->edges[3]);
    if (!(p->flame_limit >= 0.0f)) return fail(SF_EINVAL, "sf_behavior: flame_limit %g (>= 0)", (double)p->flame_limit);
    if (p->k < 0 || p->k > SF_DIST_MAX_POINTS) return fail(SF_EINVAL, "sf_behavior: %d points per environment (1..%d)", p->k, SF_DIST_MAX_POINTS);
    if (p->k > 0 && !p->points) return fail(SF_EINVAL, "sf_behavior: k = %d needs points", p->k);
    if (p->k == 0 && p->points) return fail(SF_EINVAL, "sf_behavior: points need k > 0");
    if (out->point_flame && p->k == 0) return fail(SF_EINVAL, "sf_behavior: point_flame needs k > 0");
    if (p->k > 0 && !out->point_flame) return fail(SF_EINVAL, "sf_behavior: points without point_flame");
    if (((uintptr_t)out->hpa | (uintptr_t)out->ros | (uintptr_t)out->intensity | (uintptr_t)out->flame_length | (uintptr_t)out->max_flame |
         (uintptr_t)out->max_intensity | (uintptr_t)out->classes | (uintptr_t)out->point_flame | (uintptr_t)p->points) & 3)
        return fail(SF_EINVAL, "sf_behavior: an output is not aligned to its element");
    SF_TRY(check_envs(s, "sf_behavior", n, envs));
    SF_TRY(check_ready(s, "sf_behavior", kNeedRt | kNeedReset));
    const bool per_env = s->tables.size() > 1;
    std::vector<int32_t> tabs;
    for (int i = 0; i < n; ++i) {
        const int t = per_env ? envs[i] : 0;
        if (!s->tables[t].layers)
            return fail(SF_ESTATE, "sf_behavior: environment %d's table came from sf_set_rtable: there are no layers to take the reaction intensity from", envs[i]);
        tabs.push_back(t);
    }
    SF_TRY(begin_call(s, "sf_behavior", kNeedRt | kNeedReset | kNotVoid));
    if (n == 0) return SF_OK;

    BehaviorState &b = s->behavior;
    SF_TRY(ensure_hpa(s, tabs));
    const size_t bytes = (size_t)n * sizeof(int32_t);
    SF_TRY(block_reserve(s, b.blk, bytes));
    memcpy(b.blk.pinned, envs, bytes);
    SF_TRY(block_send(s, b.blk, bytes));
    if (out->max_flame) HIPCHK(hipMemsetAsync(out->max_flame, 0, (size_t)n * sizeof(float), s->stream));
    if (out->max_intensity) HIPCHK(hipMemsetAsync(out->max_intensity, 0, (size_t)n * sizeof(float), s->stream));
    if (out->classes) HIPCHK(hipMemsetAsync(out->classes, 0, (size_t)n * 5 * sizeof(int32_t), s->stream));

    BehArgs a;
    memset(&a, 0, sizeof a);
    a.H = g.H; a.W = g.W; a.P = g.P; a.PV = g.PV;
    a.plane_env = g.plane_env; a.rt_env = g.rt_env; a.cells_env = g.cells_env;
    a.status = s->status;
    a.cells = s->bl_cur ? s->cells : nullptr;
    a.rt = s->rt;
    a.hpa = b.hpa;
    a.hpa_env = per_env ? (long long)g.H * g.W : 0;
    a.envs = reinterpret_cast<const int32_t *>(b.blk.dev);
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
    return finish_call(s, "sf_behavior", !s->async, nullptr);
}

extern "C" int sf_get_behavior_builds(sf_sim *s, int64_t *n_out)
{
    if (!s || !n_out) return fail(SF_EINVAL, "sf_get_behavior_builds: null argument");
    *n_out = s->behavior.builds;
    return SF_OK;
}
