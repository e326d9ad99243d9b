// Host code of the wind changes: sf_set_wind, the schedules and their pass in front of a stepping call.
// Part of the single translation unit simfire_hip.hip (included there, behind sf_handle.h).
#pragma once

// ----------------------------------------------------------------------------- wind changes
// The wind-independent terms of the listed tables (host list) made current in the cache plane, modelled on ensure_rtc: allocated at
// the first wind change, filled per run of stale tables.  SF_ENOTSUP: no cache (no memory for it, or switched off by the lab) - the
// caller builds from the layers.
static int ensure_wterms(sf_sim *s, const int32_t *tabs, int n)
{
    if (s->wind.cache_off) return SF_ENOTSUP;
    const Geo &g = s->g;
    const size_t n_tab = (size_t)s->tables.size(), per = (size_t)kWindPlanes * g.H * g.W;
    if (!s->wind.terms) {
        if (hipMalloc(reinterpret_cast<void **>(&s->wind.terms), per * n_tab * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); s->wind.terms = nullptr; return SF_ENOTSUP; }
        s->bytes += (int64_t)(per * n_tab * sizeof(float));
        s->tables.wterms_allocated();
    }
    std::vector<int32_t> stale;
    for (int k = 0; k < n; ++k) if (s->tables[tabs[k]].wt_stale) stale.push_back(tabs[k]);
    std::sort(stale.begin(), stale.end());
    const Thetas th = rt_thetas();
    for (size_t i = 0; i < stale.size();) {
        size_t j = i + 1;
        while (j < stale.size() && stale[j] == stale[j - 1] + 1 && j - i < 65535) ++j;
        hipLaunchKernelGGL(k_wind_terms, dim3((unsigned)((g.W + kWindThreads - 1) / kWindThreads), (unsigned)g.H, (unsigned)(j - i)), dim3(kWindThreads), 0,
                           s->stream, g.H, g.W, (const double *)s->lay_all, (const int32_t *)nullptr, (int)stale[i], s->slope_scale, (float)s->p.h,
                           (float)s->p.S_T, (float)s->p.S_e, (float)s->p.p_p, (float)s->p.M_f, th, s->wind.terms);
        for (size_t k = i; k < j; ++k) s->tables.wterms_built(stale[k]);
        i = j;
    }
    HIPCHK(hipGetLastError());
    return SF_OK;
}

// k_wind_rtable for `count` listed tables, or - cnt_dev - for as many as the device says (at most max_count); enqueue layer
static int wind_launch(sf_sim *s, const int32_t *list_dev, const uint32_t *cnt_dev, int count, int max_count, const double *U, const double *U_dir,
                       int field, bool cached)
{
    const Geo &g = s->g;
    WindArgs a;
    a.H = g.H; a.W = g.W; a.P = g.P;
    a.lay = s->lay_all; a.cache = s->wind.terms; a.rt = s->rt; a.rtc = s->rtc;
    a.tab_stride = (long long)8 * g.plane_env;
    a.list = list_dev; a.count_dev = cnt_dev; a.count = count;
    a.U = U; a.U_dir = U_dir; a.field = field;
    a.ps = s->slope_scale;
    a.h = (float)s->p.h; a.S_T = (float)s->p.S_T; a.S_e = (float)s->p.S_e; a.p_p = (float)s->p.p_p; a.M_f = (float)s->p.M_f;
    a.th = rt_thetas();
    const long long items = (long long)max_count * g.H * ((g.P + kWindThreads - 1) / kWindThreads);
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(items, (long long)s->n_cu * 8));
    if (cached) hipLaunchKernelGGL(k_wind_rtable<true>, dim3(grid), dim3(kWindThreads), 0, s->stream, a);
    else hipLaunchKernelGGL(k_wind_rtable<false>, dim3(grid), dim3(kWindThreads), 0, s->stream, a);
    HIPCHK(hipGetLastError());
    return SF_OK;
}

static void wind_sched_count(sf_sim *s)
{
    s->wind.sched.clear();
    for (int e = 0; e < (int)s->wind.K.size(); ++e) if (s->wind.K[e]) s->wind.sched.push_back(e);
    s->tables.schedule_changed();
}

// The tables of these environments were rebuilt from their layers (or their state was loaded): whichever segment a schedule built
// them for, the next stepping call decides anew.
static int wind_forget(sf_sim *s, const int32_t *envs, int n)
{
    bool any = false;
    for (int k = 0; k < n && !any; ++k) any = s->wind.sched_dev && s->wind.K[envs[k]] != 0;
    if (!any) return SF_OK;
    const int32_t *list_dev = nullptr;
    SF_TRY(block_stage(s, s->wind.blk, &list_dev, envs, (size_t)n * 4));
    hipLaunchKernelGGL(k_wind_sched_forget, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, n, list_dev, s->wind.sched_dev);
    HIPCHK(hipGetLastError());
    return SF_OK;
}

// In front of the updates of a stepping call while a schedule is set (enqueue layer): the cache made current for the scheduled
// tables, the due list made on the device, the due tables rebuilt.  Nothing is read back.
static int wind_sched_pass(sf_sim *s)
{
    const Geo &g = s->g;
    const int n = (int)s->wind.sched.size();
    bool cached = s->wind.sched_cached;
    if (!s->tables.wind_sched_ready()) {
        const int rc = ensure_wterms(s, s->wind.sched.data(), n);
        if (rc && rc != SF_ENOTSUP) return rc;
        cached = s->wind.sched_cached = rc == SF_OK;
        s->tables.schedule_ready();
    }
    SF_TRY(lab_start(s, s->wind.timer));
    HIPCHK(hipMemsetAsync(s->wind.due_cnt, 0, sizeof(uint32_t), s->stream));
    hipLaunchKernelGGL(k_wind_due, dim3((unsigned)((g.E + 255) / 256)), dim3(256), 0, s->stream, g, (const EnvState *)s->commit, (const EnvState *)s->tmp,
                       (const uint32_t *)s->flags, s->seq, s->planes.committed() ? 1 : 0, s->wind.sched_dev, s->wind.due_cnt, s->wind.due, s->wind.due_U, s->wind.due_D);
    SF_TRY(wind_launch(s, s->wind.due, s->wind.due_cnt, 0, n, s->wind.due_U, s->wind.due_D, 0, cached));
    SF_TRY(lab_stop(s, s->wind.timer));
    return SF_OK;
}

// the tables a wind call addresses: the list, or every table in order; what must hold before any device work
static int wind_targets(const sf_sim *s, const char *who, int32_t n, const int32_t *envs, bool need_per_env, std::vector<int32_t> &tabs)
{
    if (n < 0) return fail(SF_EINVAL, "%s: n = %d", who, n);
    const int n_tab = s->tables.size();
    if ((envs || need_per_env) && !s->p.per_env_terrain)
        return fail(SF_ESTATE, "%s: this handle shares one terrain between all environments (create it with per_env_terrain = 1)", who);
    if (envs) SF_TRY(check_envs(s, who, n, envs, "listed twice"));
    else if (n != 0 && n != n_tab) return fail(SF_EINVAL, "%s: without a list n must be the number of tables, %d (got %d)", who, n_tab, n);
    tabs.resize((size_t)n);
    for (int i = 0; i < n; ++i) tabs[i] = envs ? envs[i] : i;
    for (int i = 0; i < n; ++i)
        if (!s->tables[tabs[i]].layers) return fail(SF_ESTATE, "%s: table %d has no layers (sf_set_layers*, sf_generate_layers)", who, tabs[i]);
    return SF_OK;
}

// fire.py:365, 490-494: self.U / self.U_dir reassigned between two update() calls
extern "C" int sf_set_wind(sf_sim *s, int32_t n, const int32_t *envs, const double *U, const double *U_dir, int32_t flags)
{
    if (!s) return fail(SF_EINVAL, "sf_set_wind: null handle");
    if (flags & ~(SF_WIND_FIELD | SF_WIND_DEVICE)) return fail(SF_EINVAL, "sf_set_wind: unknown flags 0x%x", flags);
    if (n > 0 && (!U || !U_dir)) return fail(SF_EINVAL, "sf_set_wind: null argument");
    std::vector<int32_t> tabs;
    SF_TRY(wind_targets(s, "sf_set_wind", n, envs, false, tabs));
    if (n == 0) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const Geo &g = s->g;
    const bool field = (flags & SF_WIND_FIELD) != 0, device = (flags & SF_WIND_DEVICE) != 0;
    const size_t cells = (size_t)g.H * g.W, list_bytes = ((size_t)n * 4 + 7) / 8 * 8;
    const bool scalars = !field && !device;         // the host scalars travel behind the list
    CallBlock &blk = s->wind.blk;
    SF_TRY(block_reserve(s, blk, list_bytes + (scalars ? (size_t)n * 16 : 0)));
    memcpy(blk.pinned, tabs.data(), (size_t)n * 4);
    if (scalars) { memcpy(blk.pinned + list_bytes, U, (size_t)n * 8); memcpy(blk.pinned + list_bytes + (size_t)n * 8, U_dir, (size_t)n * 8); }
    SF_TRY(block_send(s, blk, list_bytes + (scalars ? (size_t)n * 16 : 0)));
    const int32_t *list_dev = (const int32_t *)blk.dev;
    const int rcw = ensure_wterms(s, tabs.data(), n);
    if (rcw && rcw != SF_ENOTSUP) return rcw;
    const bool cached = rcw == SF_OK;
    SF_TRY(lab_start(s, s->wind.timer));
    if (field && !device) {
        // host fields go through the stage buffer, as many tables at a time as fit 64 MB of it (one at least)
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)64 << 20) / (cells * 16)));
        SF_TRY(ensure_stage(s, (size_t)chunk * cells * 16));
        double *su = (double *)s->stage, *sd = su + (size_t)chunk * cells;
        for (int i0 = 0; i0 < n; i0 += chunk) {
            const int cnt = std::min(chunk, n - i0);
            HIPCHK(hipMemcpyAsync(su, U + (size_t)i0 * cells, (size_t)cnt * cells * 8, hipMemcpyHostToDevice, s->stream));
            HIPCHK(hipMemcpyAsync(sd, U_dir + (size_t)i0 * cells, (size_t)cnt * cells * 8, hipMemcpyHostToDevice, s->stream));
            SF_TRY(wind_launch(s, list_dev + i0, nullptr, cnt, cnt, su, sd, 1, cached));
        }
    } else {
        const double *u = scalars ? (const double *)(blk.dev + list_bytes) : U, *d = scalars ? (const double *)(blk.dev + list_bytes) + n : U_dir;
        SF_TRY(wind_launch(s, list_dev, nullptr, n, n, u, d, field ? 1 : 0, cached));
    }
    SF_TRY(lab_stop(s, s->wind.timer));
    // the direction-major table was replaced; the cell-major copy, where the buffer exists, was written in the same pass
    s->tables.wind_rebuilt(tabs.data(), n, s->rtc != nullptr);
    bool had = false;
    for (int i = 0; i < n; ++i) if (s->wind.sched_dev && s->wind.K[tabs[i]]) { had = true; s->wind.K[tabs[i]] = 0; }
    if (had) {           // a wind set by hand ends the environment's schedule
        hipLaunchKernelGGL(k_wind_sched_set, dim3((unsigned)n), dim3(SF_WIND_MAX_SEGS), 0, s->stream, n, list_dev, 0, (const sf_wind_seg *)nullptr, s->wind.sched_dev);
        HIPCHK(hipGetLastError());
        wind_sched_count(s);
    }
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_set_wind_schedule(sf_sim *s, int32_t n, const int32_t *envs, int32_t K, const sf_wind_seg *segs)
{
    const char *who = "sf_set_wind_schedule";
    if (!s) return fail(SF_EINVAL, "%s: null handle", who);
    if (K < 0 || K > SF_WIND_MAX_SEGS) return fail(SF_EINVAL, "%s: 0 .. %d segments (got %d)", who, SF_WIND_MAX_SEGS, K);
    if (s->episodes.on && (s->episodes.p.flags & SF_EP_WIND))
        return fail(SF_ESTATE, "%s: every new episode draws its wind (sf_episodes_set with SF_EP_WIND): a schedule would fight it over the table", who);
    if (n > 0 && K > 0 && !segs) return fail(SF_EINVAL, "%s: null argument", who);
    std::vector<int32_t> tabs;
    SF_TRY(wind_targets(s, who, n, envs, true, tabs));
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < K; ++k) {
            const sf_wind_seg &r = segs[(size_t)i * K + k];
            if (r.reserved != 0) return fail(SF_EINVAL, "%s: environment %d, segment %d: reserved must be 0", who, tabs[i], k);
            if (k == 0 ? r.first_update != 0 : r.first_update <= segs[(size_t)i * K + k - 1].first_update)
                return fail(SF_EINVAL, "%s: environment %d: first_update must be 0 for segment 0 and strictly increasing (segment %d: %d)", who,
                            tabs[i], k, r.first_update);
        }
    if (n == 0) return SF_OK;
    if (K == 0 && !s->wind.sched_dev) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const Geo &g = s->g;
    if (!s->wind.sched_dev) {
        SF_TRY(dev_alloc(s, &s->wind.sched_dev, (size_t)g.E));
        SF_TRY(dev_alloc(s, &s->wind.due_U, (size_t)2 * g.E));
        SF_TRY(dev_alloc(s, &s->wind.due, (size_t)g.E + 2));
        s->wind.due_D = s->wind.due_U + g.E;
        s->wind.due_cnt = reinterpret_cast<uint32_t *>(s->wind.due + g.E);
        HIPCHK(hipMemsetAsync(s->wind.sched_dev, 0, sizeof(WindSched) * g.E, s->stream));
        s->wind.K.assign((size_t)g.E, 0);
    }
    const size_t list_bytes = ((size_t)n * 4 + 7) / 8 * 8, rows_bytes = (size_t)n * K * sizeof(sf_wind_seg);
    CallBlock &blk = s->wind.blk;
    SF_TRY(block_reserve(s, blk, list_bytes + rows_bytes));
    memcpy(blk.pinned, tabs.data(), (size_t)n * 4);
    if (rows_bytes) memcpy(blk.pinned + list_bytes, segs, rows_bytes);
    SF_TRY(block_send(s, blk, list_bytes + rows_bytes));
    hipLaunchKernelGGL(k_wind_sched_set, dim3((unsigned)n), dim3(SF_WIND_MAX_SEGS), 0, s->stream, n, (const int32_t *)blk.dev, K,
                       (const sf_wind_seg *)(blk.dev + list_bytes), s->wind.sched_dev);
    HIPCHK(hipGetLastError());
    for (int i = 0; i < n; ++i) s->wind.K[tabs[i]] = K;
    wind_sched_count(s);
    return finish_call(s, nullptr, !s->async, nullptr);
}

// Laboratory (include/simfire_hip_lab.h): the cache switched off (freed; every wind change then builds from the layers) or on again;
// HIP events around the launches of every wind change and every schedule pass.
extern "C" int sf_set_wind_lab(sf_sim *s, int32_t cache_on, int32_t timed)
{
    if (!s) return fail(SF_EINVAL, "sf_set_wind_lab: null handle");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    if (!cache_on && s->wind.terms) {
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(s->wind.release_cache());
        s->bytes -= (int64_t)((size_t)kWindPlanes * s->g.H * s->g.W * (size_t)s->tables.size() * sizeof(float));
    }
    s->wind.cache_off = !cache_on;
    s->tables.schedule_changed();
    s->episodes.nocache = false;
    s->wind.timer = {timed != 0, false};
    return SF_OK;
}
extern "C" int sf_get_wind_ms(sf_sim *s, float *ms_out)
{
    if (!s || !ms_out) return fail(SF_EINVAL, "sf_get_wind_ms: null argument");
    return lab_ms(s, s->wind.timer, "sf_get_wind_ms", "no wind change or schedule pass has been timed (sf_set_wind_lab)", ms_out);
}
