// Host code of the terrain: the layers and the R tables built from them (sf_set_layers*, sf_set_rtable*, sf_generate_layers), what
// is read back of them (sf_get_attribute_data, sf_get_rtable*, sf_get_slopes).
// Part of the single translation unit simfire_hip.hip (included there, behind sf_handle.h).
#pragma once

// which R tables an env argument addresses: env < 0 = all of them
static int table_range(sf_sim *s, int env, const char *who, int *lo, int *hi)
{
    const int n_tab = s->tables.size();
    if (env < 0) { *lo = 0; *hi = n_tab; return SF_OK; }
    if (n_tab == 1) return fail(SF_ESTATE, "%s: this handle shares one terrain between all environments "
                                "(create it with per_env_terrain = 1)", who);
    if (env >= n_tab) return fail(SF_EINVAL, "%s: environment %d out of range", who, env);
    *lo = env; *hi = env + 1;
    return SF_OK;
}
// theta = arctan2(src_y - dst_y, dst_x - src_x) of the 8 travel directions, float32 (rothermel.py:102)
static Thetas rt_thetas()
{
    Thetas th;
    for (int k = 0; k < 8; ++k) th.v[k] = atan2f((float)SF_SRC_DY[k], (float)(-SF_SRC_DX[k]));
    return th;
}

// src[i] == nullptr: plane i of table `lo` is already on the device (filled from a fuel-code raster)
static int set_layers_impl(sf_sim *s, int env, const double *const src[7])
{
    int lo, hi, rc = table_range(s, env, "sf_set_layers", &lo, &hi);
    if (rc) return rc;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const Geo &g = s->g;
    const size_t n = (size_t)g.H * g.W;
    for (int i = 0; i < 7; ++i)
        if (src[i]) HIPCHK(hipMemcpyAsync(s->layer(lo, i), src[i], n * sizeof(double), hipMemcpyHostToDevice, s->stream));
    dim3 blk(256), grd((g.W + 255) / 256, g.H);
    hipLaunchKernelGGL(k_slopes, grd, blk, 0, s->stream, g.H, g.W, s->layer(lo, 4), s->slope_scale, s->smag, s->sdir);
    const Thetas th = rt_thetas();
    dim3 grd2((g.P + 255) / 256, g.H);
    const size_t tab = (size_t)8 * g.plane_env;
    hipLaunchKernelGGL(k_rtable, grd2, blk, 0, s->stream, g.H, g.W, g.P, s->layer(lo, 0), s->layer(lo, 1), s->layer(lo, 2),
                       s->layer(lo, 3), s->layer(lo, 5), s->layer(lo, 6), s->smag, s->sdir, (float)s->p.h, (float)s->p.S_T,
                       (float)s->p.S_e, (float)s->p.p_p, (float)s->p.M_f, th, s->rt + (size_t)lo * tab);
    HIPCHK(hipGetLastError());
    for (int i = lo + 1; i < hi; ++i) {   // same terrain for several environments: replicate layers and table
        HIPCHK(hipMemcpyAsync(s->layer(i, 0), s->layer(lo, 0), 7 * n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        HIPCHK(hipMemcpyAsync(s->rt + (size_t)i * tab, s->rt + (size_t)lo * tab, tab * sizeof(double),
                              hipMemcpyDeviceToDevice, s->stream));
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    const std::vector<int32_t> tabs = iota_tabs(lo, hi);
    s->tables.layers_set(tabs.data(), hi - lo, src[0] == nullptr);
    if (s->wind.sched_dev) {
        rc = wind_forget(s, tabs.data(), hi - lo);
        if (!rc && !s->wind.sched.empty()) HIPCHK(hipStreamSynchronize(s->stream));
    }
    return rc;
}

extern "C" int sf_set_layers(sf_sim *s, const double *w_0, const double *delta, const double *M_x,
                             const double *sigma, const double *elevation, const double *U, const double *U_dir)
{
    if (!s) return fail(SF_EINVAL, "sf_set_layers: null handle");
    const double *src[7] = {w_0, delta, M_x, sigma, elevation, U, U_dir};
    return set_layers_impl(s, -1, src);
}

extern "C" int sf_set_layers_env(sf_sim *s, int32_t env, const double *w_0, const double *delta, const double *M_x,
                                 const double *sigma, const double *elevation, const double *U, const double *U_dir)
{
    if (!s) return fail(SF_EINVAL, "sf_set_layers_env: null handle");
    if (env < 0) return fail(SF_EINVAL, "sf_set_layers_env: environment %d out of range", env);
    const double *src[7] = {w_0, delta, M_x, sigma, elevation, U, U_dir};
    return set_layers_impl(s, env, src);
}

// FuelLayer._get_data (simfire/utils/layers.py:670-676): FBFM13 code raster -> Fuel through the
// FuelModelToFuel table (simfire/enums.py:176-198), done on the device.  The table is the caller's.
extern "C" int sf_set_layers_fbfm(sf_sim *s, int32_t env, const int32_t *codes, int32_t n_lut, const int32_t *lut_codes,
                                  const double *lut_fuel, const double *elevation, const double *U, const double *U_dir)
{
    if (!s || !codes || !lut_codes || !lut_fuel || !elevation || !U || !U_dir)
        return fail(SF_EINVAL, "sf_set_layers_fbfm: null argument");
    if (n_lut < 1 || n_lut > kMaxFuelLut) return fail(SF_EINVAL, "sf_set_layers_fbfm: n_lut must be 1..%d", kMaxFuelLut);
    int lo, hi, rc = table_range(s, env, "sf_set_layers_fbfm", &lo, &hi);
    if (rc) return rc;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const Geo &g = s->g;
    const size_t n = (size_t)g.H * g.W;
    SF_TRY(ensure_stage(s, n * sizeof(int32_t) + (1 + kRdFbfmColours) * sizeof(int32_t)));      // codes | bad | sf_render's colour codes
    int32_t *codes_dev = (int32_t *)s->stage, *bad_dev = codes_dev + n;
    HIPCHK(hipMemcpyAsync(codes_dev, codes, n * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
    const int32_t none = INT32_MIN;
    HIPCHK(hipMemcpyAsync(bad_dev, &none, sizeof none, hipMemcpyHostToDevice, s->stream));
    FuelLut lut;
    lut.n = n_lut;
    for (int i = 0; i < n_lut; ++i) {
        lut.code[i] = lut_codes[i];
        for (int k = 0; k < 4; ++k) lut.fuel[i][k] = lut_fuel[4 * i + k];
    }
    hipLaunchKernelGGL(k_fuel_lut, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, (long long)n,
                       (const int32_t *)codes_dev, lut, s->layer(lo, 0), s->layer(lo, 1), s->layer(lo, 2), s->layer(lo, 3), bad_dev);
    HIPCHK(hipGetLastError());
    int32_t bad = none;
    HIPCHK(hipMemcpyAsync(&bad, bad_dev, sizeof bad, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (bad != none) return fail(SF_EINVAL, "sf_set_layers_fbfm: fuel model code %d is not in the table", bad);
    // the codes' colours for sf_render (FuelLayer._make_image, layers.py:654-667): the codes are dropped after the lookup above
    if (!s->render.fuel_ix) HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->render.fuel_ix), n * (size_t)s->tables.size()));
    int32_t *tab_dev = bad_dev + 1;
    HIPCHK(hipMemcpyAsync(tab_dev, kRdFbfmCodes, sizeof kRdFbfmCodes, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_render_fuel_ix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, (long long)n, (const int32_t *)codes_dev,
                       (const int32_t *)tab_dev, kRdFbfmColours, s->render.fuel_ix + (size_t)lo * n);
    HIPCHK(hipGetLastError());
    for (int i = lo + 1; i < hi; ++i)
        HIPCHK(hipMemcpyAsync(s->render.fuel_ix + (size_t)i * n, s->render.fuel_ix + (size_t)lo * n, n, hipMemcpyDeviceToDevice, s->stream));
    const double *src[7] = {nullptr, nullptr, nullptr, nullptr, elevation, U, U_dir};
    return set_layers_impl(s, env, src);
}

// FireSimulation.get_attribute_data (simfire/sim/simulation.py:376-403): w_0 / delta / M_x as float32,
// sigma as uint32 (astype truncation), elevation and wind as supplied (float64).  Null pointers are
// skipped; device_pointers != 0: the outputs are device buffers (observation tensors stay in HBM).
extern "C" int sf_get_attribute_data(sf_sim *s, int32_t env, float *w_0, uint32_t *sigma, float *delta, float *M_x,
                                     double *elevation, double *wind_speed, double *wind_direction, int32_t device_pointers)
{
    if (!s) return fail(SF_EINVAL, "sf_get_attribute_data: null handle");
    const int n_tab = s->tables.size();
    if (env < 0 || env >= s->g.E) return fail(SF_EINVAL, "sf_get_attribute_data: environment %d out of range", env);
    const int t = n_tab == 1 ? 0 : env;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const Geo &g = s->g;
    const size_t n = (size_t)g.H * g.W;
    const hipMemcpyKind kind = device_pointers ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (w_0 || sigma || delta || M_x) {
        SF_TRY(ensure_stage(s, 4 * n * sizeof(float)));
        float *st = (float *)s->stage;
        float *d_w0 = device_pointers && w_0 ? w_0 : st, *d_de = device_pointers && delta ? delta : st + 2 * n,
              *d_mx = device_pointers && M_x ? M_x : st + 3 * n;
        uint32_t *d_si = device_pointers && sigma ? sigma : (uint32_t *)(st + n);
        hipLaunchKernelGGL(k_attribute_planes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, (long long)n,
                           (const double *)s->layer(t, 0), (const double *)s->layer(t, 1), (const double *)s->layer(t, 2),
                           (const double *)s->layer(t, 3), d_w0, d_si, d_de, d_mx);
        HIPCHK(hipGetLastError());
        if (!device_pointers) {
            if (w_0) HIPCHK(hipMemcpyAsync(w_0, st, n * 4, kind, s->stream));
            if (sigma) HIPCHK(hipMemcpyAsync(sigma, st + n, n * 4, kind, s->stream));
            if (delta) HIPCHK(hipMemcpyAsync(delta, st + 2 * n, n * 4, kind, s->stream));
            if (M_x) HIPCHK(hipMemcpyAsync(M_x, st + 3 * n, n * 4, kind, s->stream));
        }
    }
    if (elevation) HIPCHK(hipMemcpyAsync(elevation, s->layer(t, 4), n * sizeof(double), kind, s->stream));
    if (wind_speed) HIPCHK(hipMemcpyAsync(wind_speed, s->layer(t, 5), n * sizeof(double), kind, s->stream));
    if (wind_direction) HIPCHK(hipMemcpyAsync(wind_direction, s->layer(t, 6), n * sizeof(double), kind, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

// sf_generate_layers (include/simfire_hip.h; sf_gen_kernels.h): every argument is checked before any device work
static int check_noise(const sf_noise &p, int e, const char *plane)
{
    if (p.kind == SF_GEN_NONE || p.kind == SF_GEN_CONSTANT) return SF_OK;
    if (p.kind != SF_GEN_SIMPLEX) return fail(SF_EINVAL, "sf_generate_layers: environment %d, %s: unknown kind %d", e, plane, p.kind);
    if (!(p.scale > 0.0)) return fail(SF_EINVAL, "sf_generate_layers: environment %d, %s: scale must be > 0", e, plane);
    if (p.octaves < 1 || p.octaves > kGenMaxOctaves)
        return fail(SF_EINVAL, "sf_generate_layers: environment %d, %s: octaves must be 1..%d", e, plane, kGenMaxOctaves);
    if (!(p.lo < p.hi)) return fail(SF_EINVAL, "sf_generate_layers: environment %d, %s: range_min must be less than range_max", e, plane);
    return SF_OK;
}

extern "C" int sf_generate_layers(sf_sim *s, int32_t n, const int32_t *envs, const sf_layer_gen *gen)
{
    if (!s) return fail(SF_EINVAL, "sf_generate_layers: null handle");
    if (n < 0) return fail(SF_EINVAL, "sf_generate_layers: n = %d", n);
    if (n > 0 && (!envs || !gen)) return fail(SF_EINVAL, "sf_generate_layers: null argument");
    if (!s->p.per_env_terrain)
        return fail(SF_ESTATE, "sf_generate_layers: this handle shares one terrain between all environments (create it with per_env_terrain = 1)");
    const Geo &g = s->g;
    SF_TRY(check_envs(s, "sf_generate_layers", n, envs, "listed twice"));
    for (int k = 0; k < n; ++k) {
        const int e = envs[k];
        const sf_layer_gen &d = gen[k];
        int rc = check_noise(d.elevation, e, "elevation");
        if (!rc) rc = check_noise(d.wind_speed, e, "wind_speed");
        if (!rc) rc = check_noise(d.wind_direction, e, "wind_direction");
        if (rc) return rc;
        if (d.fuel != SF_GEN_NONE && d.fuel != SF_GEN_CONSTANT)
            return fail(SF_EINVAL, "sf_generate_layers: environment %d, fuel: unknown kind %d", e, d.fuel);
    }
    if (n == 0) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const size_t gen_bytes = (size_t)n * sizeof(sf_layer_gen), bytes = gen_bytes + (size_t)n * sizeof(int32_t);
    CallBlock &blk = s->gen_blk;
    SF_TRY(block_reserve(s, blk, bytes));
    memcpy(blk.pinned, gen, gen_bytes);
    memcpy(blk.pinned + gen_bytes, envs, (size_t)n * sizeof(int32_t));
    SF_TRY(block_send(s, blk, bytes));
    const sf_layer_gen *gen_d = (const sf_layer_gen *)blk.dev;
    const int32_t *envs_d = (const int32_t *)(blk.dev + gen_bytes);
    const long long cells = (long long)g.H * g.W;
    const Thetas th = rt_thetas();
    for (int k0 = 0; k0 < n; k0 += kGenChunk) {          // (grid y / z hold at most kGenChunk environments)
        const int m = std::min(n - k0, kGenChunk);
        hipLaunchKernelGGL(k_gen_planes, dim3((unsigned)((cells + kGenThreads - 1) / kGenThreads), (unsigned)m, 4), dim3(kGenThreads), 0,
                           s->stream, g.H, g.W, s->lay_all, envs_d, gen_d, k0);
        HIPCHK(hipGetLastError());
    }
    for (int k0 = 0; k0 < n; k0 += kGenChunk) {
        const int m = std::min(n - k0, kGenChunk);
        hipLaunchKernelGGL(k_gen_rtable, dim3((unsigned)((g.P + kGenThreads - 1) / kGenThreads), (unsigned)g.H, (unsigned)m), dim3(kGenThreads), 0,
                           s->stream, g.H, g.W, g.P, (const double *)s->lay_all, envs_d, k0, s->slope_scale, (float)s->p.h, (float)s->p.S_T,
                           (float)s->p.S_e, (float)s->p.p_p, (float)s->p.M_f, th, s->rt, (long long)8 * g.plane_env);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    s->tables.layers_set(envs, n, false);
    return wind_forget(s, envs, n);
}

static int set_rtable_impl(sf_sim *s, int env, const double *R8)
{
    int lo, hi, rc = table_range(s, env, "sf_set_rtable", &lo, &hi);
    if (rc) return rc;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const Geo &g = s->g;
    const size_t n = (size_t)8 * g.H * g.W * sizeof(double);
    SF_TRY(ensure_stage(s, n));
    HIPCHK(hipMemcpyAsync(s->stage, R8, n, hipMemcpyHostToDevice, s->stream));
    dim3 blk(256), grd((g.P + 255) / 256, g.H, 8);
    const size_t tab = (size_t)8 * g.plane_env;
    for (int i = lo; i < hi; ++i)
        hipLaunchKernelGGL(k_pack_rt, grd, blk, 0, s->stream, g.H, g.W, g.P, (const double *)s->stage, s->rt + (size_t)i * tab);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->stream));
    s->tables.rtable_set(iota_tabs(lo, hi).data(), hi - lo);
    return SF_OK;
}

extern "C" int sf_set_rtable(sf_sim *s, const double *R8)
{
    if (!s || !R8) return fail(SF_EINVAL, "sf_set_rtable: null argument");
    return set_rtable_impl(s, -1, R8);
}

extern "C" int sf_set_rtable_env(sf_sim *s, int32_t env, const double *R8)
{
    if (!s || !R8) return fail(SF_EINVAL, "sf_set_rtable_env: null argument");
    if (env < 0) return fail(SF_EINVAL, "sf_set_rtable_env: environment %d out of range", env);
    return set_rtable_impl(s, env, R8);
}

static int get_rtable_impl(sf_sim *s, int env, double *out)
{
    const int n_tab = s->tables.size();
    const int t = n_tab == 1 ? 0 : env;
    if (t < 0 || t >= n_tab) return fail(SF_EINVAL, "sf_get_rtable: environment %d out of range", env);
    if (!s->tables[t].rt) return fail(SF_ESTATE, "sf_get_rtable: no layers / table set");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const Geo &g = s->g;
    const size_t n = (size_t)8 * g.H * g.W * sizeof(double);
    SF_TRY(ensure_stage(s, n));
    dim3 blk(256), grd((g.W + 255) / 256, g.H, 8);
    hipLaunchKernelGGL(k_unpack_f64, grd, blk, 0, s->stream, g.H, g.W, g.P,
                       (const double *)(s->rt + (size_t)t * 8 * g.plane_env), (double *)s->stage);
    HIPCHK(hipMemcpyAsync(out, s->stage, n, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

extern "C" int sf_get_rtable(sf_sim *s, double *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_rtable: null argument");
    return get_rtable_impl(s, 0, out);
}

extern "C" int sf_get_rtable_env(sf_sim *s, int32_t env, double *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_rtable_env: null argument");
    return get_rtable_impl(s, env, out);
}

extern "C" int sf_get_slopes(sf_sim *s, double *mag, double *dir)
{
    if (!s || !mag || !dir) return fail(SF_EINVAL, "sf_get_slopes: null argument");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const size_t n = (size_t)s->g.H * s->g.W * sizeof(double);
    HIPCHK(hipMemcpyAsync(mag, s->smag, n, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(dir, s->sdir, n, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}
