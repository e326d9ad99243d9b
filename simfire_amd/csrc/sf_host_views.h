// Host code of what is derived from the state without changing it: arrival times and values at risk (the passes behind the step
// launches, DESIGN.md sections 17 and 20), ensemble statistics (21), the history, observations (12) and frames (14).
// Part of the single translation unit simfire_hip.hip (included there, behind sf_handle.h).
#pragma once

// ----------------------------------------------------------------------------- arrival times
// The pass behind the launches (sf_arrival_kernels.h): reads every environment's update count from commit[], so the step rings are
// folded first.  Sparse where the blocked plane is current and every plane of the vector bitmap is known to match it, else dense over
// whichever plane is current.  Recording off: nothing.  arrival_scan: the plane alone, without the value pass behind it (a caller
// that counts the damage again from the plane anyway: ignite_rows).
static int arrival_scan(sf_sim *s)
{
    if (!s->arrival.plane) return SF_OK;
    { int rc0 = ensure_commit(s); if (rc0) return rc0; }
    const Geo &g = s->g;
    const bool sparse = s->planes.bits_cover_cells() && !s->arrival.dense;
    if (sparse) {
        hipLaunchKernelGGL(k_arrival_bits, dim3((unsigned)((g.H * g.VW + 255) / 256), (unsigned)g.E), dim3(256), 0, s->stream, g, (const uint8_t *)s->cells,
                           (const unsigned long long *)s->vbits, (const EnvState *)s->commit, s->arrival.plane);
    } else {
        const dim3 grd((unsigned)((g.W + 255) / 256), (unsigned)g.H, (unsigned)g.E), blk(256);
        const uint8_t *cells = cur_cells(s);
        if (g.ab == 1) hipLaunchKernelGGL(k_arrival_cells<uint8_t>, grd, blk, 0, s->stream, g, (const uint8_t *)s->age, cells, (const EnvState *)s->commit, s->arrival.plane);
        else if (g.ab == 2) hipLaunchKernelGGL(k_arrival_cells<uint16_t>, grd, blk, 0, s->stream, g, (const uint8_t *)s->age, cells, (const EnvState *)s->commit, s->arrival.plane);
        else hipLaunchKernelGGL(k_arrival_cells<uint32_t>, grd, blk, 0, s->stream, g, (const uint8_t *)s->age, cells, (const EnvState *)s->commit, s->arrival.plane);
    }
    HIPCHK(hipGetLastError());
    s->arrival.passes[sparse ? 0 : 1]++;
    s->arrival.pending = 0;
    return SF_OK;
}
static int arrival_pass(sf_sim *s)
{
    if (!s->arrival.plane) return SF_OK;
    SF_TRY(arrival_scan(s));
    return s->values.plane ? value_pass(s) : SF_OK;      // the plane is complete up to commit[].steps: so is the damage behind this
}
// The plane's per-environment slice behind the n slices env_segs has filled (a reset zeroes it, a fork copies it): appended here and not
// a kind of sf_env_segs.h - the plane is not one of the buffers the step kernels know.  Returns the new count.
static int arrival_seg(const sf_sim *s, EnvSeg *seg, int n)
{
    if (!s->arrival.plane) return n;
    assert(n < kEnvSegs);
    const long long len = s->g.plane_env * 4;
    seg[n] = {reinterpret_cast<uint8_t *>(s->arrival.plane), len, len};
    return n + 1;
}

// ----------------------------------------------------------------------------- values at risk
static ValueArgs value_args(const sf_sim *s)
{
    ValueArgs a;
    a.values = s->values.plane; a.values_env = s->values.per_env ? s->g.plane_env : 0;
    a.arrival1 = s->arrival.plane; a.commit = s->commit; a.rec = s->val_rec();
    return a;
}
// The pass behind the arrival pass (sf_value_kernels.h; arrival_pass has folded the step rings and completed the plane): the sum
// over the window in the sparse form under the arrival pass's own condition, else dense, then the commit of the records.
static int value_pass(sf_sim *s)
{
    const Geo &g = s->g;
    const bool sparse = s->planes.bits_cover_cells() && !s->values.dense;
    if (sparse) hipLaunchKernelGGL(k_value_bits, dim3((unsigned)((g.H * g.VW + 255) / 256), (unsigned)g.E), dim3(256), 0, s->stream, g,
                                   (const unsigned long long *)s->vbits, value_args(s));
    else hipLaunchKernelGGL(k_value_cells, dim3((unsigned)((g.W + 255) / 256), (unsigned)g.H, (unsigned)g.E), dim3(256), 0, s->stream, g, value_args(s));
    hipLaunchKernelGGL(k_value_commit, dim3((unsigned)((g.E + 255) / 256)), dim3(256), 0, s->stream, g.E, (const EnvState *)s->commit, s->val_rec());
    HIPCHK(hipGetLastError());
    s->values.passes[sparse ? 0 : 1]++;
    return SF_OK;
}
// Every record from the arrival plane as it stands (sf_values_set, sf_load_state): records of zeros, then the dense form once over
// every environment - by the invariant exact for all of them.  A handle that was never reset has nothing to count.
static int value_recount(sf_sim *s)
{
    if (!s->values.plane) return SF_OK;
    const Geo &g = s->g;
    HIPCHK(hipMemsetAsync(s->val_rec(), 0, (size_t)g.E * sizeof(ValueRec), s->stream));
    if (!s->planes.was_reset()) return SF_OK;
    if (s->arrival.pending) return arrival_pass(s);       // (a call that failed half way left updates behind: the plane first, the pass behind it counts)
    SF_TRY(ensure_commit(s));
    hipLaunchKernelGGL(k_value_cells, dim3((unsigned)((g.W + 255) / 256), (unsigned)g.H, (unsigned)g.E), dim3(256), 0, s->stream, g, value_args(s));
    hipLaunchKernelGGL(k_value_commit, dim3((unsigned)((g.E + 255) / 256)), dim3(256), 0, s->stream, g.E, (const EnvState *)s->commit, s->val_rec());
    HIPCHK(hipGetLastError());
    s->values.passes[1]++;
    return SF_OK;
}
// The record's slice behind the arrival plane's (a reset zeroes it: upto1 == 0, the pass behind the reset sums the ignition; a fork
// copies it with the plane): appended like arrival_seg.  Returns the new count.
static int value_seg(const sf_sim *s, EnvSeg *seg, int n)
{
    if (!s->values.plane) return n;
    assert(n < kEnvSegs);
    seg[n] = {reinterpret_cast<uint8_t *>(s->val_rec()), (long long)sizeof(ValueRec), (long long)sizeof(ValueRec)};
    return n + 1;
}
static int value_free(sf_sim *s)
{
    if (!s->values.plane) return SF_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    s->bytes -= (int64_t)(s->val_plane_bytes() + s->val_aux_bytes());
    HIPCHK(s->values.release());
    s->values.w_on = false;
    return SF_OK;
}

extern "C" int sf_values_set(sf_sim *s, const int32_t *values, int32_t per_env, int32_t device_pointer)
{
    if (!s) return fail(SF_EINVAL, "sf_values_set: null handle");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    if (!values) return value_free(s);
    if (!s->arrival.plane) return fail(SF_ESTATE, "sf_values_set: call sf_enable_arrival first (the arrival plane says which cells count)");
    const Geo &g = s->g;
    const size_t n_planes = per_env ? (size_t)g.E : 1, rows = n_planes * g.H, cells = rows * g.W;
    if (!device_pointer)
        for (size_t i = 0; i < cells; ++i)
            if (values[i] > kValueMax || values[i] < -kValueMax)
                return fail(SF_EINVAL, "sf_values_set: value %d (entry %lld) is outside -2^24 .. 2^24", values[i], (long long)i);
    SF_TRY(check_team_error(s, "sf_values_set"));
    // the new plane and, the first time, the records: made and checked before the handle changes (a refused call leaves it as it was)
    int32_t *plane = nullptr;
    uint8_t *aux = s->values.aux;
    const size_t plane_bytes = rows * g.P * sizeof(int32_t);
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&plane), plane_bytes));
    if (!aux && hipMalloc(reinterpret_cast<void **>(&aux), s->val_aux_bytes()) != hipSuccess) { (void)hipFree(plane); return fail(SF_EHIP, "sf_values_set: hipMalloc failed"); }
    hipError_t err = hipMemsetAsync(aux, 0, s->val_aux_bytes(), s->stream);      // (records and ticks start from zero under a new plane)
    if (err == hipSuccess) err = hipMemsetAsync(plane, 0, plane_bytes, s->stream);
    if (err == hipSuccess) err = hipMemcpy2DAsync(plane, (size_t)g.P * 4, values, (size_t)g.W * 4, (size_t)g.W * 4, rows,
                                                  device_pointer ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream);
    uint32_t bad = 0;
    if (err == hipSuccess && device_pointer) {
        uint32_t *word = reinterpret_cast<uint32_t *>(aux + (size_t)g.E * (sizeof(ValueRec) + 16));
        hipLaunchKernelGGL(k_value_range, dim3((unsigned)std::min<size_t>((cells + 255) / 256, 4096)), dim3(256), 0, s->stream, values, (long long)cells, word);
        err = hipGetLastError();
        if (err == hipSuccess) err = hipMemcpyAsync(&bad, word, sizeof bad, hipMemcpyDeviceToHost, s->stream);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(s->stream);      // (the caller's memory is free again; kernels that read the old plane are through)
    if (err != hipSuccess || bad) {
        (void)hipFree(plane);
        if (!s->values.aux) (void)hipFree(aux);
        else if (s->planes.was_reset()) (void)value_recount(s);      // (the records were zeroed above: counted again under the plane that stays)
        if (bad) return fail(SF_EINVAL, "sf_values_set: a value of the device plane is outside -2^24 .. 2^24");
        return fail(SF_EHIP, "sf_values_set: %s", hipGetErrorString(err));
    }
    if (s->values.plane) { s->bytes -= (int64_t)s->val_plane_bytes(); HIPCHK(hipFree(s->values.plane)); }
    else s->bytes += (int64_t)s->val_aux_bytes();
    s->values.plane = plane; s->values.aux = aux; s->values.per_env = per_env != 0;
    s->bytes += (int64_t)s->val_plane_bytes();
    SF_TRY(value_recount(s));
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_values_get(sf_sim *s, int64_t *damage_out)
{
    if (!s || !damage_out) return fail(SF_EINVAL, "sf_values_get: null argument");
    if (!s->values.plane) return fail(SF_ESTATE, "sf_values_get: call sf_values_set first");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipMemcpy2DAsync(damage_out, 8, s->val_rec(), sizeof(ValueRec), 8, (size_t)s->g.E, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return check_team_error(s, "sf_values_get");
}

extern "C" int sf_values_device(sf_sim *s, void **damage, int64_t *damage_stride, void **tick_loss)
{
    if (!s || !damage || !damage_stride || !tick_loss) return fail(SF_EINVAL, "sf_values_device: null argument");
    if (!s->values.plane) return fail(SF_ESTATE, "sf_values_device: call sf_values_set first");
    *damage = s->val_rec(); *damage_stride = (int64_t)sizeof(ValueRec); *tick_loss = s->val_tick(1);
    return SF_OK;
}

extern "C" int sf_values_set_weight(sf_sim *s, float w_value, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_values_set_weight: null handle");
    if (!s->agents.p.k) return fail(SF_ESTATE, "sf_values_set_weight: call sf_agents_create first");
    if (!s->values.plane) return fail(SF_ESTATE, "sf_values_set_weight: call sf_values_set first");
    s->values.w = w_value; s->values.w_on = on != 0;
    return SF_OK;
}

extern "C" int sf_set_values_dense(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_set_values_dense: null handle");
    s->values.dense = on != 0;
    return SF_OK;
}

extern "C" int sf_get_value_passes(sf_sim *s, int64_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_value_passes: null argument");
    out[0] = s->values.passes[0]; out[1] = s->values.passes[1];
    return SF_OK;
}

// ----------------------------------------------------------------------------- ensemble statistics
// One launch of k_ensemble (sf_ensemble_kernels.h) over the arrival plane as it stands: the call converts no plane, folds no ring and
// looks at no result row - it reads arrival1 (complete behind every stepping call) and the value plane, and writes the caller's outputs.
template <int TP>
static void ensemble_launch(bool loss, dim3 grd, hipStream_t st, const EnsArgs &a)
{
    if (loss) hipLaunchKernelGGL((k_ensemble<TP, true>), grd, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_ensemble<TP, false>), grd, dim3(256), 0, st, a);
}

extern "C" int sf_ensemble_stats(sf_sim *s, const sf_ensemble_params *p, const int32_t *members, const sf_ensemble_out *out)
{
    if (!s || !p || !members || !out) return fail(SF_EINVAL, "sf_ensemble_stats: null argument");
    if (!out->count && !out->prob && !out->first && !out->mean && !out->loss) return fail(SF_EINVAL, "sf_ensemble_stats: no output asked for");
    const Geo &g = s->g;
    const int G = p->n_groups, K = p->group_size, T = p->n_horizons;
    if (G < 1 || K < 1 || K > 65535 || (long long)G * K > (1LL << 20))
        return fail(SF_EINVAL, "sf_ensemble_stats: %d groups of %d members (G >= 1, 1 <= K <= 65535, G * K <= 2^20)", G, K);
    if (T < 1 || T > SF_ENS_MAX_HORIZONS) return fail(SF_EINVAL, "sf_ensemble_stats: %d horizons (1..%d)", T, SF_ENS_MAX_HORIZONS);
    if (p->reserved != 0) return fail(SF_EINVAL, "sf_ensemble_stats: reserved must be 0");
    for (int t = 0; t < T; ++t) {
        const int h = p->horizons[t];
        if (h < -1 || (h == -1 && t != T - 1)) return fail(SF_EINVAL, "sf_ensemble_stats: horizon %d is %d (>= 0; -1, no limit, only last)", t, h);
        if (t > 0 && h != -1 && h <= p->horizons[t - 1]) return fail(SF_EINVAL, "sf_ensemble_stats: the horizons are not strictly ascending (%d behind %d)", h, p->horizons[t - 1]);
    }
    if (((uintptr_t)out->count | (uintptr_t)out->prob | (uintptr_t)out->first | (uintptr_t)out->mean) & 3 || ((uintptr_t)out->loss & 7))
        return fail(SF_EINVAL, "sf_ensemble_stats: an output is not aligned to its element");
    SF_TRY(check_envs(s, "sf_ensemble_stats", G * K, members));
    if (!s->arrival.plane) return fail(SF_ESTATE, "sf_ensemble_stats: call sf_enable_arrival first (the statistics are read off the arrival plane)");
    if (out->loss && !s->values.plane) return fail(SF_ESTATE, "sf_ensemble_stats: loss needs a value plane (sf_values_set)");
    SF_TRY(begin_call(s, "sf_ensemble_stats", kNotVoid));

    EnsArgs a;
    memset(&a, 0, sizeof a);
    SF_TRY(block_stage(s, s->ens_blk, &a.members, members, (size_t)G * K * sizeof(int32_t)));
    a.arrival1 = s->arrival.plane; a.plane_env = g.plane_env;
    a.H = g.H; a.W = g.W; a.P = g.P; a.Q = (g.W + 3) / 4;
    a.G = G; a.K = K; a.T = T;
    int TP = 1;
    while (TP < T) TP *= 2;
    for (int t = 0; t < SF_ENS_MAX_HORIZONS; ++t) {
        const int h = p->horizons[std::min(t, T - 1)];
        a.hz[t] = h < 0 ? 0xFFFFFFFEu : (uint32_t)h;
    }
    if (out->loss) { a.values = s->values.plane; a.values_env = s->values.per_env ? g.plane_env : 0; }
    a.vec = g.W % 4 == 0 && !(((uintptr_t)out->count | (uintptr_t)out->prob | (uintptr_t)out->first | (uintptr_t)out->mean) & 15);
    a.count = out->count; a.prob = out->prob; a.first = out->first; a.mean = out->mean;
    a.loss = reinterpret_cast<unsigned long long *>(out->loss);
    if (out->loss) HIPCHK(hipMemsetAsync(out->loss, 0, (size_t)G * T * sizeof(int64_t), s->stream));
    const long long quads = (long long)g.H * a.Q;
    const dim3 grd((unsigned)((quads + 255) / 256), (unsigned)std::min(G, kEnsGroupsY), (unsigned)((G + kEnsGroupsY - 1) / kEnsGroupsY));
    const bool loss = out->loss != nullptr;
    if (TP == 1) ensemble_launch<1>(loss, grd, s->stream, a);
    else if (TP == 2) ensemble_launch<2>(loss, grd, s->stream, a);
    else if (TP == 4) ensemble_launch<4>(loss, grd, s->stream, a);
    else ensemble_launch<8>(loss, grd, s->stream, a);
    return finish_call(s, "sf_ensemble_stats", !s->async, nullptr);
}

// The per-update history FireSimulation._save_data appends to fire_map.npy (simulation.py:548-549,
// 887-959: int8 [T, H, W], one map after every executed update), recorded on the device.
extern "C" int sf_enable_history(sf_sim *s, int32_t capacity)
{
    if (!s) return fail(SF_EINVAL, "sf_enable_history: null handle");
    if (capacity < 0) return fail(SF_EINVAL, "sf_enable_history: capacity must be >= 0");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t per = (size_t)s->g.E * s->g.H * s->g.W;
    if (s->history) { HIPCHK(hipFree(s->history)); s->bytes -= (int64_t)(per * s->history_cap); }
    s->history = nullptr; s->history_cap = 0;
    if (capacity == 0) return SF_OK;
    HIPCHK(hipMalloc((void **)&s->history, per * capacity));
    s->bytes += (int64_t)(per * capacity);
    s->history_cap = capacity;
    HIPCHK(hipMemsetAsync(s->history, 0, per * capacity, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

extern "C" int sf_get_history(sf_sim *s, int32_t env, int32_t first, int32_t count, int8_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_history: null argument");
    if (!s->history) return fail(SF_ESTATE, "sf_get_history: call sf_enable_history first");
    if (env < 0 || env >= s->g.E) return fail(SF_EINVAL, "sf_get_history: environment %d out of range", env);
    if (first < 0 || count < 0 || count > s->history_cap)
        return fail(SF_EINVAL, "sf_get_history: %d updates from %d do not fit the capacity %d", count, first, s->history_cap);
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const size_t map = (size_t)s->g.H * s->g.W;
    const int8_t *base = s->history + (size_t)env * s->history_cap * map;
    const int slot = first % s->history_cap;
    const int n1 = count < s->history_cap - slot ? count : s->history_cap - slot;    // up to the end of the ring
    if (n1) HIPCHK(hipMemcpyAsync(out, base + (size_t)slot * map, (size_t)n1 * map, hipMemcpyDeviceToHost, s->stream));
    if (count > n1) HIPCHK(hipMemcpyAsync(out + (size_t)n1 * map, base, (size_t)(count - n1) * map, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

extern "C" int sf_history_device(sf_sim *s, void **ptr, int32_t *capacity)
{
    if (!s || !ptr || !capacity) return fail(SF_EINVAL, "sf_history_device: null argument");
    *ptr = s->history; *capacity = s->history_cap;
    return SF_OK;
}

// Arrival times: which update created the first sprite of a cell (fire.py:571-587), kept by a pass behind the
// step launches (arrival_pass; enqueue_call cuts a call into pieces of at most max_fire_duration updates while this is on).
extern "C" int sf_enable_arrival(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_enable_arrival: null handle");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const size_t n = (size_t)s->g.E * s->g.plane_env;
    if (!on) {
        if (!s->arrival.plane) return SF_OK;
        if (s->values.plane) return fail(SF_ESTATE, "sf_enable_arrival: a value plane is set and needs the arrival plane: switch it off first (sf_values_set with NULL)");
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(s->arrival.release());
        s->bytes -= (int64_t)(n * sizeof(uint32_t));
        return SF_OK;
    }
    if (s->arrival.plane) return SF_OK;
    SF_TRY(dev_alloc(s, &s->arrival.plane, n));
    HIPCHK(hipMemsetAsync(s->arrival.plane, 0, n * sizeof(uint32_t), s->stream));
    s->arrival.pending = 0;
    if (s->planes.was_reset()) SF_TRY(arrival_pass(s));      // the sprites that are live now carry their true updates
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_get_arrival(sf_sim *s, int32_t env, int32_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_arrival: null argument");
    if (!s->arrival.plane) return fail(SF_ESTATE, "sf_get_arrival: call sf_enable_arrival first");
    const Geo &g = s->g;
    if (env < 0 || env >= g.E) return fail(SF_EINVAL, "sf_get_arrival: environment %d out of range", env);
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipMemcpy2DAsync(out, (size_t)g.W * 4, s->arrival.plane + (size_t)env * g.plane_env, (size_t)g.P * 4, (size_t)g.W * 4, (size_t)g.H,
                            hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    SF_TRY(check_team_error(s, "sf_get_arrival"));
    for (size_t i = 0, n = (size_t)g.H * g.W; i < n; ++i) out[i] -= 1;      // stored: update + 1, 0 = never
    return SF_OK;
}

extern "C" int sf_arrival_device(sf_sim *s, void **ptr, int64_t *row_pitch, int64_t *env_stride)
{
    if (!s || !ptr || !row_pitch || !env_stride) return fail(SF_EINVAL, "sf_arrival_device: null argument");
    if (!s->arrival.plane) return fail(SF_ESTATE, "sf_arrival_device: call sf_enable_arrival first");
    *ptr = s->arrival.plane; *row_pitch = (int64_t)s->g.P * 4; *env_stride = (int64_t)s->g.plane_env * 4;
    return SF_OK;
}

extern "C" int sf_set_arrival_dense(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_set_arrival_dense: null handle");
    s->arrival.dense = on != 0;
    return SF_OK;
}

extern "C" int sf_time_arrival_pass(sf_sim *s, float *ms_out)
{
    if (!s || !ms_out) return fail(SF_EINVAL, "sf_time_arrival_pass: null argument");
    if (!s->arrival.plane) return fail(SF_ESTATE, "sf_time_arrival_pass: call sf_enable_arrival first");
    SF_TRY(begin_call(s, "sf_time_arrival_pass", kCommit));      // (the commit is not part of the pass's time)
    HIPCHK(hipEventRecord(s->ev0, s->stream));
    SF_TRY(arrival_pass(s));
    return finish_call(s, nullptr, true, ms_out);
}

extern "C" int sf_get_arrival_passes(sf_sim *s, int64_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_arrival_passes: null argument");
    out[0] = s->arrival.passes[0]; out[1] = s->arrival.passes[1];
    return SF_OK;
}

// ----------------------------------------------------------------------------- observations
extern "C" int sf_cell_layout(sf_sim *s, int32_t *blocked)
{
    if (!s || !blocked) return fail(SF_EINVAL, "sf_cell_layout: null argument");
    *blocked = s->planes.blocked() ? 1 : 0;
    return SF_OK;
}

// Output cells per k_observe workgroup (TX x TY) for pool factor f and output width ow, and the LDS row stride of its staged region:
// up to 256 outputs, fewer as f grows, so that the region (TY * f rows of whole vectors) fits kObsLds.
struct ObsTile { int TX, TY, stride; };
static ObsTile obs_tile(int f, int ow)
{
    int outs = kObsThreads;
    while (outs > 1 && (long long)outs * f * f > 16384) outs >>= 1;
    for (;;) {
        int tx = 1;
        while (tx * 2 <= outs && tx * 2 <= 64 && tx < ow) tx *= 2;
        ObsTile t{tx, outs / tx, (tx * f + 30) / 16 * 16};
        if ((long long)t.TY * f * t.stride <= kObsLds || outs == 1) return t;
        outs >>= 1;
    }
}

extern "C" int sf_observe(sf_sim *s, const sf_obs_params *p, int32_t n, const int32_t *envs, void *device_out)
{
    if (!s || !p) return fail(SF_EINVAL, "sf_observe: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && (!envs || !device_out))) return fail(SF_EINVAL, "sf_observe: bad environment list or output");
    const int C = p->n_channels;
    if (C < 1 || C > SF_OBS_MAX_CHANNELS) return fail(SF_EINVAL, "sf_observe: %d channels (1..%d)", C, SF_OBS_MAX_CHANNELS);
    bool attr = false, agents = false;
    for (int c = 0; c < C; ++c) {
        if (p->channels[c] < SF_OBS_FIRE_MAP || p->channels[c] > SF_OBS_AGENTS)
            return fail(SF_EINVAL, "sf_observe: channel %d has the unknown code %d", c, p->channels[c]);
        if (p->pool_mode[c] != 0 && p->pool_mode[c] != 1) return fail(SF_EINVAL, "sf_observe: channel %d has the pool mode %d (0 mean, 1 max)", c, p->pool_mode[c]);
        attr |= p->channels[c] >= SF_OBS_W_0 && p->channels[c] <= SF_OBS_WIND_DIRECTION;
        agents |= p->channels[c] == SF_OBS_AGENTS;
    }
    const int f = p->pool;
    if (f < 1 || f > SF_OBS_MAX_POOL) return fail(SF_EINVAL, "sf_observe: pool %d (1..%d)", f, SF_OBS_MAX_POOL);
    const bool crop = p->crop_h != 0 || p->crop_w != 0;
    if (crop && (p->crop_h < 1 || p->crop_w < 1 || p->crop_h > 65535 || p->crop_w > 65535))
        return fail(SF_EINVAL, "sf_observe: crop %d x %d", p->crop_h, p->crop_w);
    if (crop && !p->centers) return fail(SF_EINVAL, "sf_observe: a crop needs centers");
    const int eh = crop ? p->crop_h : g.H, ew = crop ? p->crop_w : g.W;
    if (eh % f || ew % f) return fail(SF_EINVAL, "sf_observe: the extent %d x %d is not divisible by pool %d", eh, ew, f);
    if (p->dtype != 0 && p->dtype != 1) return fail(SF_EINVAL, "sf_observe: dtype %d (0 float32, 1 bfloat16)", p->dtype);
    const int k = agents && p->agents ? p->agents_k : 0;
    if (agents && p->agents && (p->agents_k < 0 || p->agents_k > SF_OBS_MAX_AGENTS))
        return fail(SF_EINVAL, "sf_observe: %d agents per environment (0..%d)", p->agents_k, SF_OBS_MAX_AGENTS);
    if ((uintptr_t)device_out & (p->dtype ? 1 : 3)) return fail(SF_EINVAL, "sf_observe: the output is not aligned to its element");
    SF_TRY(check_envs(s, "sf_observe", n, envs));
    if (n == 0) return SF_OK;
    if (attr && !s->tables.have_rt()) return fail(SF_ESTATE, "sf_observe: attribute channels need the layers (sf_set_layers)");
    SF_TRY(begin_call(s, "sf_observe", kNotVoid));
    const int oh = eh / f, ow = ew / f;
    const ObsTile tl = obs_tile(f, ow);
    const long long tiles_x = (ow + tl.TX - 1) / tl.TX, tiles = tiles_x * ((oh + tl.TY - 1) / tl.TY);
    if ((long long)n * tiles > 0x7FFFFFFFLL) return fail(SF_ENOTSUP, "sf_observe: %d environments x %lld tiles exceed the launch grid", n, tiles);

    // the per-call block: ObsHead | envs [n] | centers [n][2] (host) | agents [n][k][3] (host)
    const size_t o_envs = (sizeof(ObsHead) + 15) / 16 * 16, o_cen = o_envs + ((size_t)n * 4 + 15) / 16 * 16;
    const bool cen_host = crop && !p->centers_device, ag_host = k > 0 && !p->agents_device;
    const size_t o_ag = o_cen + (cen_host ? ((size_t)n * 8 + 15) / 16 * 16 : 0);
    const size_t bytes = o_ag + (ag_host ? (size_t)n * k * 12 : 0);
    CallBlock &blk = s->obs_blk;
    SF_TRY(block_reserve(s, blk, bytes));
    ObsHead h;
    memset(&h, 0, sizeof h);
    for (int c = 0; c < C; ++c) { h.code[c] = p->channels[c]; h.mode[c] = p->pool_mode[c]; }
    // get_attribute_bounds (simulation.py:334-374; FuelConstants / ElevationConstants / WindConstants, enums.py:118-173) in the order of
    // supported_attributes (simulation.py:317-332)
    const double lo[7] = {0.0, 1.0, 0.2, 0.12, -282.0, 0.0, 0.0}, hi[7] = {1.0, 3500.0, 6.0, 1.0, 11000.0, 250.0, 360.0};
    for (int a = 0; a < 7; ++a) { h.lo[a] = lo[a]; h.span[a] = hi[a] - lo[a]; }
    memcpy(blk.pinned, &h, sizeof h);
    memcpy(blk.pinned + o_envs, envs, (size_t)n * 4);
    if (cen_host) memcpy(blk.pinned + o_cen, p->centers, (size_t)n * 8);
    if (ag_host) memcpy(blk.pinned + o_ag, p->agents, (size_t)n * k * 12);
    SF_TRY(block_send(s, blk, bytes));

    ObsArgs a;
    memset(&a, 0, sizeof a);
    a.g = g;
    a.pl = cur_planes(s);
    a.lay = s->lay_all;
    a.lay_tab = (size_t)s->tables.size() > 1 ? 7LL * g.H * g.W : 0;
    a.head = reinterpret_cast<const ObsHead *>(blk.dev);
    a.envs = reinterpret_cast<const int32_t *>(blk.dev + o_envs);
    a.centers = !crop ? nullptr : (cen_host ? reinterpret_cast<const int32_t *>(blk.dev + o_cen) : p->centers);
    a.agents = k == 0 ? nullptr : (ag_host ? reinterpret_cast<const int32_t *>(blk.dev + o_ag) : p->agents);
    a.out = device_out;
    a.n = n; a.C = C; a.f = f; a.ch = eh; a.cw = ew; a.oh = oh; a.ow = ow; a.k = k;
    a.TX = tl.TX; a.TY = tl.TY; a.tiles_x = (int)tiles_x; a.stride = tl.stride;
    a.norm = p->normalize != 0; a.bf16 = p->dtype == 1; a.pad = p->pad;
    hipLaunchKernelGGL(k_observe, dim3((unsigned)((long long)n * tiles)), dim3(kObsThreads), 0, s->stream, a);
    return finish_call(s, "sf_observe", !s->async, nullptr);
}

// ----------------------------------------------------------------------------- frames
// Output rows per k_render workgroup and its LDS bytes: the staged source rows (R * scale rows of P bytes) and the output bytes of the
// band (channels last: one segment of R * ow * 3 bytes, else three of R * ow), each segment with 16 bytes of alignment slack.
struct RenderTile { int R, st_bytes, out_seg, lds; };
static RenderTile render_tile(const Geo &g, int scale, int oh, int ow, bool cl)
{
    constexpr int kBudget = 32768, kMax = 65536 - 256;
    const auto make = [&](int R) {
        RenderTile t;
        t.R = R;
        t.st_bytes = (R * scale * g.P + 15) / 16 * 16;
        t.out_seg = cl ? (R * ow * 3 + 16 + 15) / 16 * 16 : (R * ow + 16 + 15) / 16 * 16;
        t.lds = t.st_bytes + (cl ? 1 : 3) * t.out_seg;
        return t;
    };
    int R = 1;
    while (R < oh && make(R + 1).lds <= kBudget) ++R;
    RenderTile t = make(R);
    if (t.lds > kMax) t.R = 0;
    return t;
}

extern "C" int sf_render(sf_sim *s, const sf_render_params *p, int32_t n, const int32_t *envs, void *device_out)
{
    if (!s || !p) return fail(SF_EINVAL, "sf_render: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && (!envs || !device_out))) return fail(SF_EINVAL, "sf_render: bad environment list or output");
    if (p->source != SF_RENDER_CURRENT && p->source != SF_RENDER_HISTORY)
        return fail(SF_EINVAL, "sf_render: source %d (0 current, 1 history)", p->source);
    const bool hist = p->source == SF_RENDER_HISTORY;
    if (hist && (p->first < 0 || p->count < 1)) return fail(SF_EINVAL, "sf_render: history frames %d from %d", p->count, p->first);
    if (p->scale < 1 || p->scale > SF_RENDER_MAX_SCALE) return fail(SF_EINVAL, "sf_render: scale %d (1..%d)", p->scale, SF_RENDER_MAX_SCALE);
    if (p->mode < SF_RENDER_NEAREST || p->mode > SF_RENDER_SPRITES) return fail(SF_EINVAL, "sf_render: mode %d (0 nearest, 1 mean, 2 sprites)", p->mode);
    if (p->background != SF_RENDER_FUEL && p->background != SF_RENDER_WHITE)
        return fail(SF_EINVAL, "sf_render: background %d (0 fuel, 1 white)", p->background);
    if (p->contours != 0 && p->contours != 1) return fail(SF_EINVAL, "sf_render: contours %d (0 or 1)", p->contours);
    if (p->channels_last != 0 && p->channels_last != 1) return fail(SF_EINVAL, "sf_render: channels_last %d (0 or 1)", p->channels_last);
    for (int c = 0; c < 3; ++c)
        if (p->terrain_rgb[c] < 0 || p->terrain_rgb[c] > 255) return fail(SF_EINVAL, "sf_render: terrain_rgb[%d] = %d (0..255)", c, p->terrain_rgb[c]);
    const int k = p->agents ? p->agents_k : 0;
    if (p->agents && (p->agents_k < 0 || p->agents_k > SF_RENDER_MAX_AGENTS))
        return fail(SF_EINVAL, "sf_render: %d agents per environment (0..%d)", p->agents_k, SF_RENDER_MAX_AGENTS);
    SF_TRY(check_envs(s, "sf_render", n, envs));
    const int s_ = p->scale, oh = (g.H + s_ - 1) / s_, ow = (g.W + s_ - 1) / s_;
    const bool cl = p->channels_last != 0;
    const RenderTile tl = render_tile(g, s_, oh, ow, cl);
    if (tl.R == 0) return fail(SF_ENOTSUP, "sf_render: a row of %d cells does not fit one workgroup's LDS", g.W);
    const int count = hist ? p->count : 1;
    const long long frames = (long long)n * count, bands = (oh + tl.R - 1) / tl.R;
    if (frames * bands > 0x7FFFFFFFLL) return fail(SF_ENOTSUP, "sf_render: %lld frames x %lld bands exceed the launch grid", frames, bands);
    if (hist && !s->history) return fail(SF_ESTATE, "sf_render: a history source needs sf_enable_history");
    if (hist && p->count > s->history_cap)
        return fail(SF_EINVAL, "sf_render: %d updates do not fit the history capacity %d", p->count, s->history_cap);
    const int n_tab = s->tables.size();
    for (int i = 0; i < n; ++i)
        if (!s->tables[n_tab == 1 ? 0 : envs[i]].layers) return fail(SF_ESTATE, "sf_render: environment %d has no layers (sf_set_layers)", envs[i]);
    if (n == 0) return SF_OK;
    SF_TRY(begin_call(s, "sf_render", kNotVoid));

    // which backgrounds to (re)build: the listed environments' stale tables; every functional one when the fuel colours were made
    // from another terrain_rgb (only the fuel background shows them)
    const int64_t rgb = p->terrain_rgb[0] | p->terrain_rgb[1] << 8 | p->terrain_rgb[2] << 16;
    if (p->background == SF_RENDER_FUEL && rgb != s->render.rgb) {
        s->tables.rgb_changed();
        s->render.rgb = rgb;
    }
    std::vector<int32_t> tabs, fb;
    {
        std::vector<char> want(n_tab, 0);
        for (int i = 0; i < n; ++i) want[n_tab == 1 ? 0 : envs[i]] = 1;
        for (int t = 0; t < n_tab; ++t)
            if (want[t] && s->tables[t].bg_stale) { tabs.push_back(t); fb.push_back(s->tables[t].fbfm); }
    }
    if (!s->render.bg) HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->render.bg), (size_t)n_tab * g.H * g.W * sizeof(uint32_t)));

    // the per-call block: envs [n] | tabs [nt] | fbfm [nt] | min / max [nt][2] | agents [n][k][3] (host)
    const int nt = (int)tabs.size();
    const auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    const bool ag_host = k > 0 && !p->agents_device;
    const size_t o_tabs = up16((size_t)n * 4), o_fb = o_tabs + up16((size_t)nt * 4), o_mm = o_fb + up16((size_t)nt * 4);
    const size_t o_ag = o_mm + (size_t)nt * 16, bytes = o_ag + (ag_host ? (size_t)n * k * 12 : 0);
    CallBlock &blk = s->render.blk;
    SF_TRY(block_reserve(s, blk, bytes));
    memcpy(blk.pinned, envs, (size_t)n * 4);
    if (nt) { memcpy(blk.pinned + o_tabs, tabs.data(), (size_t)nt * 4); memcpy(blk.pinned + o_fb, fb.data(), (size_t)nt * 4); }
    if (ag_host) memcpy(blk.pinned + o_ag, p->agents, (size_t)n * k * 12);
    // (the lists, and the agents behind the min / max words: those are the kernels' to write)
    SF_TRY(block_send(s, blk, o_mm, o_ag, ag_host ? (size_t)n * k * 12 : 0));

    if (nt) {
        RenderBgArgs b;
        memset(&b, 0, sizeof b);
        b.H = g.H; b.W = g.W;
        b.lay = s->lay_all; b.lay_tab = 7LL * g.H * g.W;
        b.fuel_ix = s->render.fuel_ix;
        b.tabs = reinterpret_cast<const int32_t *>(blk.dev + o_tabs);
        b.fbfm = reinterpret_cast<const int32_t *>(blk.dev + o_fb);
        b.mm = reinterpret_cast<double *>(blk.dev + o_mm);
        b.bg = s->render.bg;
        b.base = (uint32_t)(s->render.rgb < 0 ? rgb : s->render.rgb);
        for (int c = 0; c < kRdFbfmColours; ++c) {
            uint32_t w = 0;
            for (int ch = 0; ch < 3; ++ch) w |= (uint32_t)(uint8_t)(kRdFbfmRgb[c][ch] * 255.0) << (8 * ch);     // astype(np.uint8)
            b.fbfm_rgb[c] = w;
        }
        hipLaunchKernelGGL(k_render_minmax, dim3((unsigned)nt), dim3(1024), 0, s->stream, b);
        hipLaunchKernelGGL(k_render_bg, dim3((unsigned)g.H, (unsigned)nt), dim3(kRdThreads), 0, s->stream, b);
        HIPCHK(hipGetLastError());
        for (int t : tabs) s->tables.background_built(t);
    }

    RenderArgs a;
    memset(&a, 0, sizeof a);
    a.g = g;
    a.pl = cur_planes(s);
    if (hist) a.pl.cells = nullptr;      // (the history ring is the source: neither plane is read)
    a.hist = hist ? s->history : nullptr;
    a.cap = s->history_cap; a.first = hist ? p->first : 0; a.count = count;
    a.bg = s->render.bg;
    a.bg_tab = n_tab > 1 ? (long long)g.H * g.W : 0;
    a.envs = reinterpret_cast<const int32_t *>(blk.dev);
    a.agents = k == 0 ? nullptr : (ag_host ? reinterpret_cast<const int32_t *>(blk.dev + o_ag) : p->agents);
    a.out = static_cast<uint8_t *>(device_out);
    a.n_frames = (int)frames; a.k = k;
    a.s = s_; a.mode = p->mode; a.white = p->background == SF_RENDER_WHITE; a.contours = p->contours; a.cl = cl;
    a.oh = oh; a.ow = ow; a.R = tl.R; a.stride = g.P; a.st_bytes = tl.st_bytes; a.out_seg = tl.out_seg;
    hipLaunchKernelGGL(k_render, dim3((unsigned)(frames * bands)), dim3(kRdThreads), (unsigned)tl.lds, s->stream, a);
    return finish_call(s, "sf_render", !s->async, nullptr);
}
