// Host code of the environment state as a whole: fork, snapshot and restore and the resets (section 15).
// Part of the single translation unit simfire_hip.hip (included there, behind sf_handle.h).
#pragma once

// ----------------------------------------------------------------------------- environment state
// Every state call begins as begin_call(kStateCall): the closed loop ended, a reset insisted on, a voided handle refused, the step
// rings folded into commit[].

extern "C" int sf_copy_envs(sf_sim *s, const int32_t *src, const int32_t *dst, int32_t n, int32_t flags)
{
    if (!s) return fail(SF_EINVAL, "sf_copy_envs: null handle");
    if (n < 0 || (n > 0 && (!src || !dst))) return fail(SF_EINVAL, "sf_copy_envs: bad environment lists");
    if (flags & ~SF_COPY_TERRAIN) return fail(SF_EINVAL, "sf_copy_envs: unknown flags 0x%x", flags);
    const Geo &g = s->g;
    std::vector<char> role((size_t)g.E, 0);       // bit 0: a source, bit 1: a destination
    { int rc = check_envs(s, "sf_copy_envs", n, src); if (!rc) rc = check_envs(s, "sf_copy_envs", n, dst); if (rc) return rc; }
    for (int i = 0; i < n; ++i) {
        if (role[dst[i]] & 2) return fail(SF_EINVAL, "sf_copy_envs: environment %d is a destination twice", dst[i]);
        role[dst[i]] |= 2;
    }
    for (int i = 0; i < n; ++i) role[src[i]] |= 1;
    for (int e = 0; e < g.E; ++e)
        if (role[e] == 3) return fail(SF_EINVAL, "sf_copy_envs: environment %d is both a source and a destination", e);
    if (n == 0) return SF_OK;
    SF_TRY(begin_call(s, "sf_copy_envs", kStateCall));
    // Every per-environment slice of the current layout and of the structures derived from it: a handle-wide "rebuild" flag would make
    // the next step rebuild them for every environment.
    CopyList L;
    const bool terrain = (flags & SF_COPY_TERRAIN) && (size_t)s->tables.size() > 1;      // (a stale rtc copy stays marked stale below)
    // (section 20: the record travels with the arrival plane it was summed over - under ONE plane for all environments.  Planes per
    // environment stay where they are, like the terrain without SF_COPY_TERRAIN: dst's damage is its own plane over src's arrival,
    // recounted below)
    L.n_seg = arrival_seg(s, L.seg, env_segs(s, terrain ? kForkKinds : kForkKinds & ~kSegTerrain, L.seg));
    if (!s->values.per_env) L.n_seg = value_seg(s, L.seg, L.n_seg);
    const unsigned gx = seg_grid_x(L.seg, L.n_seg);
    // with the terrain go the slices of section 18, where they exist: the table's part of the wind cache, the environment's schedule
    // and the segment its table stands for (a launch of their own: the slice table of env_segs is full)
    CopyList Wl;
    Wl.n_seg = 0;
    if (terrain && s->wind.terms) Wl.seg[Wl.n_seg++] = {reinterpret_cast<uint8_t *>(s->wind.terms), (long long)kWindPlanes * g.H * g.W * 4, (long long)kWindPlanes * g.H * g.W * 4};
    if (terrain && s->wind.sched_dev) Wl.seg[Wl.n_seg++] = {reinterpret_cast<uint8_t *>(s->wind.sched_dev), (long long)sizeof(WindSched), (long long)sizeof(WindSched)};
    for (int i0 = 0; i0 < n; i0 += kCopyPairs) {
        const int cnt = std::min(kCopyPairs, n - i0);
        for (int i = 0; i < cnt; ++i) { L.src[i] = Wl.src[i] = src[i0 + i]; L.dst[i] = Wl.dst[i] = dst[i0 + i]; }
        hipLaunchKernelGGL(k_env_copy, dim3(gx, (unsigned)cnt), dim3(256), 0, s->stream, L);
        if (Wl.n_seg) hipLaunchKernelGGL(k_env_copy, dim3(seg_grid_x(Wl.seg, Wl.n_seg), (unsigned)cnt), dim3(256), 0, s->stream, Wl);
        HIPCHK(hipGetLastError());
    }
    for (int i = 0; i < n; ++i) {
        if (s->delta.snap) s->delta.snap_valid[dst[i]] = 0;      // (sf_get_fire_map_delta: the next query for dst hands back the whole map once)
        if (terrain) {
            s->tables.copied(dst[i], src[i], s->rtc != nullptr);
            if (s->render.fuel_ix && s->tables[src[i]].fbfm && dst[i] != src[i]) {
                const size_t cells = (size_t)g.H * g.W;
                HIPCHK(hipMemcpyAsync(s->render.fuel_ix + (size_t)dst[i] * cells, s->render.fuel_ix + (size_t)src[i] * cells, cells,
                                      hipMemcpyDeviceToDevice, s->stream));
            }
            if (s->wind.sched_dev) s->wind.K[dst[i]] = s->wind.K[src[i]];
        }
    }
    if (terrain && s->wind.sched_dev) wind_sched_count(s);
    if (s->values.per_env) SF_TRY(value_recount(s));
    // (the book's fire_rows bounds every environment's fire, dst's copy included; its row_fresh: dst's row is src's current row)
    return finish_call(s, nullptr, !s->async, nullptr);
}

static StateHeader state_header(const sf_sim *s)
{
    const Geo &g = s->g;
    StateHeader h;
    memset(&h, 0, sizeof h);
    h.magic = kStateMagic; h.version = kStateVersion;
    h.bytes = state_layout(g, s->parents != nullptr, s->arrival.plane != nullptr).bytes;
    h.H = g.H; h.W = g.W; h.md = g.md; h.ab = g.ab;
    h.diag = g.diag; h.att = g.att; h.has_max_time = g.has_max_time; h.prune_after_quit = g.prune_after_quit;
    h.has_parents = s->parents != nullptr; h.fire_rows = s->planes.fire_rows(); h.has_arrival = s->arrival.plane != nullptr;
    h.max_time = g.has_max_time ? g.max_time : 0.0; h.update_rate = g.update_rate; h.pixel_scale = g.pixel_scale;
    return h;
}

// a blob this handle can take: every value its state depends on matches (the first one that does not is named)
static int header_check(const sf_sim *s, const StateHeader &b, int i)
{
    const StateHeader h = state_header(s);
    const char *what = nullptr;
    if (b.magic != h.magic) what = "magic number (not a state blob)";
    else if (b.version != h.version) what = "format version";
    else if (b.H != h.H || b.W != h.W) what = "grid size";
    else if (b.md != h.md || b.ab != h.ab) what = "max_fire_duration";
    else if (b.diag != h.diag) what = "diagonal spread";
    else if (b.att != h.att) what = "line attenuation";
    else if (b.has_max_time != h.has_max_time || b.max_time != h.max_time) what = "max_time";
    else if (b.update_rate != h.update_rate) what = "update_rate";
    else if (b.pixel_scale != h.pixel_scale) what = "pixel_scale threshold";
    else if (b.prune_after_quit != h.prune_after_quit) what = "prune_after_quit";
    else if (b.has_parents != h.has_parents) what = "spread graph";
    else if (b.has_arrival != h.has_arrival) what = "arrival recording";
    else if (b.bytes != h.bytes) what = "size";
    if (what) return fail(SF_EINVAL, "sf_load_state: blob %d does not match this handle: %s", i, what);
    return SF_OK;
}

static int state_list(const sf_sim *s, int32_t n, const int32_t *envs, const void *buf, int32_t device_pointer, const char *who, bool distinct)
{
    if (n < 0 || (n > 0 && (!envs || !buf))) return fail(SF_EINVAL, "%s: bad argument", who);
    if (device_pointer && ((uintptr_t)buf & 15))      // (the kernels read / write the f64 and u32 sections in place)
        return fail(SF_EINVAL, "%s: a device buffer must be 16-byte aligned", who);
    return check_envs(s, who, n, envs, distinct ? "is listed twice" : nullptr);
}

static StateArgs state_args(sf_sim *s)
{
    StateArgs a;
    memset(&a, 0, sizeof a);
    a.g = s->g;
    a.pl = cur_planes_mut(s); a.age = s->age;
    a.burn = s->burn; a.settled = s->settled; a.parents = s->parents; a.arrival = s->arrival.plane; a.vbits = s->vbits;
    a.commit = s->commit; a.res_block = s->status_block; a.res_sink = s->sink; a.res_elapsed = s->elapsed_dev;
    a.lay = state_layout(s->g, s->parents != nullptr, s->arrival.plane != nullptr);
    a.stride = a.lay.bytes;
    return a;
}
// environments per launch, and per pass through the staging buffer of a host-pointer call (<= 64 MB of blobs unless one is larger)
static int state_chunk(const StateArgs &a, bool device)
{
    if (device) return kStateEnvs;
    return (int)std::max<long long>(1, std::min<long long>(kStateEnvs, (64LL << 20) / a.stride));
}

// ----------------------------------------------------------------------------- resets
// The two launches of a reset, the one way an environment gets a new episode: every environment taken is written in the layout that is
// current.  envs_dev: the list form's environments (distinct), else the mask form over all of them.  full: the list names every
// environment (sf_reset), so the handle-wide bookkeeping starts afresh too.
static int reset_launch(sf_sim *s, const int32_t *envs_dev, const uint8_t *mask, const int32_t *xy_dev, int n, bool full = false)
{
    const Geo &g = s->g;
    ResetArgs a;
    memset(&a, 0, sizeof a);
    a.g = g;
    const bool seams = !s->planes.blocked() && g.ab == 1;       // (the tile bookkeeping is not kept while the blocked plane is current: PlaneBook)
    // the tile histograms of a reset environment are known (all UNBURNED, the ignition's tile to be recounted); a partial reset leaves
    // it at that while every histogram of the handle is marked stale anyway
    const bool hist_known = g.ab == 1 && !s->generic && (full || !s->planes.hist_all_stale());
    if (full) s->cost_steps = 0;       // the old episodes' costs (run_cost, zeroed) say nothing
    a.n_seg = value_seg(s, a.seg, arrival_seg(s, a.seg, env_segs(s, (kResetKinds & ~(seams ? 0u : kSegSeam) & ~(hist_known ? 0u : kSegHist)) | (full ? kSegCost : 0u), a.seg)));
    a.envs = envs_dev; a.mask = mask; a.xy = xy_dev; a.n = n;
    a.pl = cur_planes_mut(s); a.age = s->age;
    a.commit = s->commit; a.tflags = s->tflags; a.ring = s->ring; a.vbits = s->vbits; a.win_hint = s->win_hint;
    a.seam = seams ? s->seam : nullptr;
    a.tdirty = hist_known ? s->tdirty : nullptr;
    a.res_block = s->status_block; a.res_sink = s->sink; a.res_elapsed = s->elapsed_dev;
    const unsigned gx = seg_grid_x(a.seg, a.n_seg);
    SF_TRY(lab_start(s, s->reset_timer));
    // Whole buffers of a large batch: a memset per slice.  Each costs a few microseconds to enqueue and clears ~14 % faster than the
    // kernel - C3's 2.7 GB in 0.46 ms against 0.50, 1 x 64 x 64 in 59 us against 30 (profiles/reset_paths_ab.txt): even at ~1 GB
    long long bytes = 0;
    for (int k = 0; k < a.n_seg; ++k) bytes += g.E * a.seg[k].len;
    if (full && bytes >= (1LL << 30)) {
        for (int k = 0; k < a.n_seg; ++k) {
            assert(a.seg[k].stride == a.seg[k].len);
            HIPCHK(hipMemsetAsync(a.seg[k].base, 0, (size_t)(g.E * a.seg[k].len), s->stream));
        }
    } else {
        hipLaunchKernelGGL(k_reset_envs, dim3(gx, (unsigned)n), dim3(256), 0, s->stream, a);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_reset_ignite, dim3((n + 255) / 256), dim3(256), 0, s->stream, a);
    HIPCHK(hipGetLastError());
    SF_TRY(lab_stop(s, s->reset_timer));
    s->planes.reset_written(full, hist_known);      // (a full one: every result row is written)
    return arrival_pass(s);             // the ignitions are the sprites of update 0 (recording off: nothing)
}
// Host ignitions: every one on the grid, or SF_EINVAL in the words of the entry `who` (envs: whose they are, null = 0 .. n - 1).
static int check_ignitions(const sf_sim *s, const char *who, int n, const int32_t *envs, const int32_t *xy)
{
    const Geo &g = s->g;
    for (int i = 0; i < n; ++i)
        if (xy[2 * i] < 0 || xy[2 * i] >= g.W || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= g.H)
            return fail(SF_EINVAL, "%s: ignition (%d, %d) of environment %d is outside the %dx%d grid", who, xy[2 * i], xy[2 * i + 1],
                        envs ? envs[i] : i, g.H, g.W);
    return SF_OK;
}
// The list form from host memory: m distinct environments and their ignitions through the call block, then the launches.
// (sf_get_fire_map_delta: a reset map is all UNBURNED - the caller zeroes its mirror, the next delta reports the ignition)
static int reset_list(sf_sim *s, const int32_t *envs, const int32_t *xy, int m, bool full = false)
{
    const int32_t *dev = nullptr;
    SF_TRY(block_stage(s, s->rs_blk, &dev, envs, (size_t)m * 4, xy, (size_t)m * 8));
    SF_TRY(reset_launch(s, dev, nullptr, dev + m, m, full));
    if (s->delta.snap) for (int i = 0; i < m; ++i) s->delta.snap_valid[envs[i]] = 1;
    return SF_OK;
}

// Every environment, as the list 0 .. E - 1 (without a mask the mask form takes only those that are not running).  Allowed before any
// reset and on a handle a failed team launch has voided; waits whatever `async` says.
extern "C" int sf_reset(sf_sim *s, const int32_t *init_xy)
{
    if (!s || !init_xy) return fail(SF_EINVAL, "sf_reset: null argument");
    const int E = s->g.E;
    SF_TRY(check_ignitions(s, "reset", E, nullptr, init_xy));
    SF_TRY(begin_call(s, "sf_reset", kCommit));
    // everything is rewritten, nothing to convert: into the blocked plane if the resident launch is what steps this handle
    // (it did last, or nothing has stepped yet and it is the automatic choice), else into the row-major planes
    const bool bl = prefers_bl(s) && (s->planes.blocked() || s->planes.last_kind() == 2 || s->planes.last_kind() == -1);
    if (bl) SF_TRY(alloc_bl(s));
    s->planes.reset_layout(bl);
    std::vector<int32_t> all((size_t)E);
    for (int e = 0; e < E; ++e) all[e] = e;
    SF_TRY(reset_list(s, all.data(), init_xy, E, true));
    SF_TRY(finish_call(s, nullptr, true, nullptr));
    s->last_ign.assign(init_xy, init_xy + (size_t)2 * E);      // (where a new episode ignites when sf_episodes_set draws no ignition)
    s->planes.reset_done();            // every environment freshly written
    if (s->team.xerr_pinned) *s->team.xerr_pinned = 0;      // (cells, bitmaps, states of every environment are new: what a failed team launch left is gone)
    return SF_OK;
}

// One environment: a list of one.  Never refused on a voided handle, and it waits whatever `async` says.
extern "C" int sf_reset_env(sf_sim *s, int32_t env, int32_t x, int32_t y)
{
    if (!s) return fail(SF_EINVAL, "sf_reset_env: null handle");
    if (env < 0 || env >= s->g.E) return fail(SF_EINVAL, "sf_reset_env: environment %d out of range", env);
    if (!s->planes.was_reset()) return fail(SF_ESTATE, "sf_reset_env: call sf_reset once first");
    const int32_t xy[2] = {x, y};
    SF_TRY(check_ignitions(s, "reset", 1, &env, xy));
    SF_TRY(begin_call(s, "sf_reset_env", kCommit));
    SF_TRY(reset_list(s, &env, xy, 1));
    return finish_call(s, nullptr, true, nullptr);
}

extern "C" int sf_time_resets(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_time_resets: null handle");
    s->reset_timer = {on != 0, false};
    return SF_OK;
}

extern "C" int sf_get_reset_ms(sf_sim *s, float *ms_out)
{
    if (!s || !ms_out) return fail(SF_EINVAL, "sf_get_reset_ms: null argument");
    return lab_ms(s, s->reset_timer, "sf_get_reset_ms", "no batched reset has been timed (sf_time_resets)", ms_out);
}

extern "C" int sf_reset_envs(sf_sim *s, int32_t n, const int32_t *envs, const int32_t *xy)
{
    if (!s) return fail(SF_EINVAL, "sf_reset_envs: null handle");
    if (n < 0 || (n > 0 && (!envs || !xy))) return fail(SF_EINVAL, "sf_reset_envs: bad environment list");
    SF_TRY(check_envs(s, "sf_reset_envs", n, envs));      // (a repeated environment is accepted: below)
    SF_TRY(check_ignitions(s, "sf_reset_envs", n, envs, xy));
    if (n == 0) return SF_OK;
    SF_TRY(begin_call(s, "sf_reset_envs", kStateCall));
    // an environment named twice keeps the last ignition given for it: no two entries of the launch write one environment
    std::vector<int32_t> last((size_t)s->g.E, -1), le, lxy;
    for (int i = 0; i < n; ++i) last[envs[i]] = i;
    for (int i = 0; i < n; ++i)
        if (last[envs[i]] == i) { le.push_back(envs[i]); lxy.push_back(xy[2 * i]); lxy.push_back(xy[2 * i + 1]); }
    SF_TRY(reset_list(s, le.data(), lxy.data(), (int)le.size()));
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_reset_where(sf_sim *s, const uint8_t *device_mask, const int32_t *xy, int32_t xy_device_pointer)
{
    if (!s) return fail(SF_EINVAL, "sf_reset_where: null handle");
    if (!xy) return fail(SF_EINVAL, "sf_reset_where: null ignitions");
    const Geo &g = s->g;
    SF_TRY(begin_call(s, "sf_reset_where", kStateCall));
    const int32_t *xy_dev = xy;
    if (!xy_device_pointer) SF_TRY(block_stage(s, s->rs_blk, &xy_dev, xy, (size_t)g.E * 8));
    SF_TRY(reset_launch(s, nullptr, device_mask, xy_dev, g.E));
    // which environments were taken is known on the device only: no host mirror of a map can be told to zero itself, so the next
    // delta query of every environment hands back the whole map once
    if (s->delta.snap) std::fill(s->delta.snap_valid.begin(), s->delta.snap_valid.end(), 0);
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_state_bytes(sf_sim *s, int64_t *bytes_out)
{
    if (!s || !bytes_out) return fail(SF_EINVAL, "sf_state_bytes: null argument");
    *bytes_out = state_layout(s->g, s->parents != nullptr, s->arrival.plane != nullptr).bytes;
    return SF_OK;
}

extern "C" int sf_save_state(sf_sim *s, int32_t n, const int32_t *envs, void *out, int32_t device_pointer)
{
    if (!s) return fail(SF_EINVAL, "sf_save_state: null handle");
    SF_TRY(state_list(s, n, envs, out, device_pointer, "sf_save_state", false));
    if (n == 0) return SF_OK;
    SF_TRY(begin_call(s, "sf_save_state", kStateCall));
    // the result rows travel with the state: made current as a status query would, but a snapshot is not a look at the result of a
    // single update (no note_result_look: the run(1)-loop heuristic stays as it was)
    SF_TRY(refresh_status(s, nullptr));
    StateArgs a = state_args(s);
    a.hdr = state_header(s);
    const int chunk = state_chunk(a, device_pointer != 0);
    if (!device_pointer) SF_TRY(ensure_stage(s, (size_t)chunk * a.stride));
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int cnt = std::min(chunk, n - i0);
        a.n = cnt;
        for (int i = 0; i < cnt; ++i) a.env[i] = envs[i0 + i];
        uint8_t *dst = device_pointer ? static_cast<uint8_t *>(out) + (size_t)i0 * a.stride : static_cast<uint8_t *>(s->stage);
        a.blob = dst;
        hipLaunchKernelGGL(k_state_pack, dim3((unsigned)((a.g.W + 255) / 256), (unsigned)a.g.H, (unsigned)cnt), dim3(256), 0, s->stream, a);
        HIPCHK(hipGetLastError());
        if (!device_pointer) {
            HIPCHK(hipMemcpyAsync(static_cast<uint8_t *>(out) + (size_t)i0 * a.stride, s->stage, (size_t)cnt * a.stride, hipMemcpyDeviceToHost, s->stream));
            HIPCHK(hipStreamSynchronize(s->stream));
        }
    }
    if (device_pointer && !s->async) HIPCHK(hipStreamSynchronize(s->stream));
    return check_team_error(s, "sf_save_state");
}

extern "C" int sf_load_state(sf_sim *s, int32_t n, const int32_t *envs, const void *in, int32_t device_pointer)
{
    if (!s) return fail(SF_EINVAL, "sf_load_state: null handle");
    SF_TRY(state_list(s, n, envs, in, device_pointer, "sf_load_state", true));
    if (n == 0) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device));
    const long long bytes = state_layout(s->g, s->parents != nullptr, s->arrival.plane != nullptr).bytes;
    // every header is looked at before anything changes (a refused call leaves the handle as it was)
    std::vector<StateHeader> hdr((size_t)n);
    if (device_pointer) {
        LOOP_QUIESCE(s);
        HIPCHK(hipMemcpy2DAsync(hdr.data(), sizeof(StateHeader), in, (size_t)bytes, sizeof(StateHeader), (size_t)n, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));      // (the blobs may come from a save enqueued in front)
    } else {
        for (int i = 0; i < n; ++i) memcpy(&hdr[i], static_cast<const uint8_t *>(in) + (size_t)i * bytes, sizeof(StateHeader));
    }
    int bound = 0;                     // the largest bound on a fire's rows the blobs carry (INT32_MAX: one carries none)
    for (int i = 0; i < n; ++i) {
        SF_TRY(header_check(s, hdr[i], i));
        bound = std::max(bound, hdr[i].fire_rows > 0 ? hdr[i].fire_rows : INT32_MAX);
    }
    SF_TRY(begin_call(s, "sf_load_state", kStateCall));
    const Geo &g = s->g;
    StateArgs a = state_args(s);
    const int chunk = state_chunk(a, device_pointer != 0);
    if (!device_pointer) SF_TRY(ensure_stage(s, (size_t)chunk * a.stride));
    const bool per_env_tiles = s->planes.tiles_kept();      // the tile maps / seams are kept: rebuild this environment's
    const bool recount = g.ab == 1 && !s->generic && !s->planes.hist_all_stale();
    EnvSeg seg[kEnvSegs];
    const int n_seg = env_segs(s, kSegCells | kSegHint, seg);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int cnt = std::min(chunk, n - i0);
        a.n = cnt;
        for (int i = 0; i < cnt; ++i) a.env[i] = envs[i0 + i];
        if (device_pointer) a.blob = const_cast<uint8_t *>(static_cast<const uint8_t *>(in)) + (size_t)i0 * a.stride;
        else {
            HIPCHK(hipMemcpyAsync(s->stage, static_cast<const uint8_t *>(in) + (size_t)i0 * a.stride, (size_t)cnt * a.stride, hipMemcpyHostToDevice, s->stream));
            a.blob = static_cast<uint8_t *>(s->stage);
        }
        for (int i = 0; i < cnt; ++i) {      // the cell planes start from zero: guard rows / quads and the pitch padding stay zero; so does the window advice (about a fire that is not there)
            const int e = a.env[i];
            for (int k = 0; k < n_seg; ++k) HIPCHK(hipMemsetAsync(seg[k].base + e * seg[k].stride, 0, (size_t)seg[k].len, s->stream));
            if (recount) HIPCHK(hipMemsetAsync(s->tdirty + (size_t)e * g.TY * g.TX, 1, (size_t)g.TY * g.TX, s->stream));
        }
        hipLaunchKernelGGL(k_state_unpack, dim3((unsigned)((g.P + 255) / 256), (unsigned)g.H, (unsigned)cnt), dim3(256), 0, s->stream, a);
        hipLaunchKernelGGL(k_state_vbits, dim3((unsigned)g.VW, (unsigned)g.H, (unsigned)cnt), dim3(64), 0, s->stream, a);
        HIPCHK(hipGetLastError());
        if (per_env_tiles)
            for (int i = 0; i < cnt; ++i) {
                int rc = rebuild_tflags(s, a.env[i], 1);
                if (!rc) rc = rebuild_seams(s, a.env[i], 1);
                if (rc) return rc;
            }
        if (!device_pointer) HIPCHK(hipStreamSynchronize(s->stream));      // (the staging buffer is reused by the next pass)
    }
    SF_TRY(wind_forget(s, envs, n));      // (a scheduled environment's table stands for the update count it had: decided anew)
    for (int i = 0; i < n; ++i) if (s->delta.snap) s->delta.snap_valid[envs[i]] = 0;
    // the bound on the fires' rows covers every environment: the saving handle's covers a loaded one (a blob without one makes it unknown)
    s->planes.state_loaded(bound != INT32_MAX ? bound : 0);
    SF_TRY(value_recount(s));      // section 20: the restored planes say what counts
    if (device_pointer && !s->async) HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}
