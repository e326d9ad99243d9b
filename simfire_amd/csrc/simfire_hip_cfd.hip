// Fifth translation unit of libsimfire_hip.so: the CFD wind solver (sf_cfd_* of include/simfire_hip.h) - kernel in
// sf_cfd_kernels.h, host side here.  Nothing of the fire-spread path is shared beyond the error message of sf_last_error.
//
// Replaces (reference mitrefireline/simfire v2.0.1): WindControllerCFD + Fluid (simfire/world/wind_mechanics/
// wind_controller.py:100-185, cfd_wind.py:8-60) and the training loop of generate_cfd_wind_layer
// (simfire/utils/generate_cfd_wind_layer.py:83-105), batched over environments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../include/simfire_hip.h"
#include "../../include/simfire_hip_lab.h"
#include "sf_cfd_kernels.h"

int sf_fail_message(int code, const char *msg);  // simfire_hip.hip: sets the message of sf_last_error

namespace {

int cfail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return sf_fail_message(code, buf);
}

#define CFDCHK(expr)                                                                                                  \
    do {                                                                                                              \
        hipError_t _e = (expr);                                                                                       \
        if (_e != hipSuccess)                                                                                         \
            return cfail(SF_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);         \
    } while (0)

// Work of one launch is bounded: about 2^24 cell updates (a Fluid.step() touches every cell ~ 3 * result_accuracy + 12
// times), at least one step.
int steps_per_launch(int n, int itr)
{
    const double per_step = (double)n * n * (3.0 * itr + 12.0);
    return (int)std::max(1.0, std::min(1e6, (double)(1 << 24) / per_step));
}

}  // namespace

struct sf_cfd {
    sf_cfd_params p;
    int device;
    hipStream_t stream;
    double *planes;  // Vx, Vy, Vx0, Vy0: [4][E][N][N]
    uint8_t *mask;   // [E][N][N]
    int *err;
    size_t plane;    // E * N * N
};

extern "C" int sf_cfd_create(const sf_cfd_params *p, sf_cfd **out)
{
    if (!p || !out) return cfail(SF_EINVAL, "sf_cfd_create: null argument");
    *out = nullptr;
    if (p->n < 4) return cfail(SF_ESHAPE, "sf_cfd_create: n = %d, the grid needs at least 4 x 4 cells", p->n);
    if (p->n > CFD_MAX_N) return cfail(SF_ENOTSUP, "sf_cfd_create: n = %d > %d", p->n, CFD_MAX_N);
    if (p->n_envs < 1) return cfail(SF_EINVAL, "sf_cfd_create: n_envs = %d", p->n_envs);
    if (p->result_accuracy < 0) return cfail(SF_EINVAL, "sf_cfd_create: result_accuracy = %d", p->result_accuracy);
    if (p->direction < 0 || p->direction > 3) return cfail(SF_EINVAL, "sf_cfd_create: direction = %d (0..3)", p->direction);
    sf_cfd *h = new sf_cfd();
    h->p = *p;
    h->plane = (size_t)p->n_envs * p->n * p->n;
    hipError_t e = hipGetDevice(&h->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&h->planes), 4 * h->plane * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&h->mask), h->plane);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&h->err), sizeof(int));
    if (e == hipSuccess) e = hipMemsetAsync(h->planes, 0, 4 * h->plane * sizeof(double), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->mask, 0, h->plane, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->err, 0, sizeof(int), h->stream);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_cfd), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)cfd_lds_bytes(CFD_MAX_N));
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        sf_cfd_destroy(h);
        return cfail(SF_EHIP, "sf_cfd_create: %s", hipGetErrorString(e));
    }
    *out = h;
    return SF_OK;
}

extern "C" int sf_cfd_destroy(sf_cfd *h)
{
    if (!h) return SF_OK;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->planes) hipFree(h->planes);
    if (h->mask) hipFree(h->mask);
    if (h->err) hipFree(h->err);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
    return SF_OK;
}

extern "C" int sf_cfd_set_terrain(sf_cfd *h, int32_t env, const uint8_t *mask)
{
    if (!h || !mask) return cfail(SF_EINVAL, "sf_cfd_set_terrain: null argument");
    if (env < -1 || env >= h->p.n_envs) return cfail(SF_EINVAL, "sf_cfd_set_terrain: env %d out of range", env);
    const size_t nn = (size_t)h->p.n * h->p.n;
    for (size_t q = 0; q < nn; ++q)
        if (mask[q] > 1) return cfail(SF_EINVAL, "sf_cfd_set_terrain: mask values are 0 or 1");
    CFDCHK(hipSetDevice(h->device));
    const int e0 = env < 0 ? 0 : env, e1 = env < 0 ? h->p.n_envs : env + 1;
    for (int e = e0; e < e1; ++e) CFDCHK(hipMemcpyAsync(h->mask + (size_t)e * nn, mask, nn, hipMemcpyHostToDevice, h->stream));
    CFDCHK(hipStreamSynchronize(h->stream));
    return SF_OK;
}

static int cfd_step(sf_cfd *h, int32_t n_steps, int32_t inflow_every, float *ms_out)
{
    if (!h) return cfail(SF_EINVAL, "sf_cfd_step: null handle");
    if (n_steps < 0) return cfail(SF_EINVAL, "sf_cfd_step: n_steps = %d", n_steps);
    CFDCHK(hipSetDevice(h->device));
    const sf_cfd_params &p = h->p;
    const int N = p.n;
    CfdArgs A;
    A.vx = h->planes;
    A.vy = h->planes + h->plane;
    A.vx0 = h->planes + 2 * h->plane;
    A.vy0 = h->planes + 3 * h->plane;
    A.mask = h->mask;
    A.err = h->err;
    A.n = N;
    A.itr = p.result_accuracy;
    A.direction = p.direction;
    A.inflow_every = inflow_every;
    A.a_diff = ((p.timestep_dt * p.viscosity) * (double)(N - 2)) * (double)(N - 2);  // cfd_wind.py:205
    A.cr_diff = 1.0 / (1.0 + 6.0 * A.a_diff);                                          // :206, :177
    A.cr_proj = 1.0 / 6.0;                                                             // :235
    A.dtx = p.timestep_dt * (double)(N - 2);                                           // :259
    A.speed = p.speed;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (ms_out) {
        CFDCHK(hipEventCreate(&ev0));
        CFDCHK(hipEventCreate(&ev1));
        CFDCHK(hipEventRecord(ev0, h->stream));
    }
    const int chunk = steps_per_launch(N, p.result_accuracy);
    for (int k0 = 0; k0 < n_steps; k0 += chunk) {
        A.k0 = k0;
        A.n_steps = std::min(chunk, n_steps - k0);
        hipLaunchKernelGGL(k_cfd, dim3(p.n_envs), dim3(CFD_THREADS), cfd_lds_bytes(N), h->stream, A);
        CFDCHK(hipGetLastError());
    }
    if (ms_out) CFDCHK(hipEventRecord(ev1, h->stream));
    CFDCHK(hipStreamSynchronize(h->stream));
    if (ms_out) {
        CFDCHK(hipEventElapsedTime(ms_out, ev0, ev1));
        hipEventDestroy(ev0);
        hipEventDestroy(ev1);
    }
    int err = 0;
    CFDCHK(hipMemcpy(&err, h->err, sizeof err, hipMemcpyDeviceToHost));
    if (err) return cfail(SF_EHIP, "sf_cfd_step: a wavefront wait of the Gauss-Seidel pass ran out; the fields are invalid");
    return SF_OK;
}

extern "C" int sf_cfd_step(sf_cfd *h, int32_t n_steps, int32_t inflow_every) { return cfd_step(h, n_steps, inflow_every, nullptr); }

extern "C" int sf_cfd_step_timed(sf_cfd *h, int32_t n_steps, int32_t inflow_every, float *ms_out)
{
    if (!ms_out) return cfail(SF_EINVAL, "sf_cfd_step_timed: null ms_out");
    return cfd_step(h, n_steps, inflow_every, ms_out);
}

extern "C" int sf_cfd_get_velocity(sf_cfd *h, int32_t env, double *vx, double *vy)
{
    if (!h) return cfail(SF_EINVAL, "sf_cfd_get_velocity: null handle");
    if (env < 0 || env >= h->p.n_envs) return cfail(SF_EINVAL, "sf_cfd_get_velocity: env %d out of range", env);
    CFDCHK(hipSetDevice(h->device));
    const size_t nn = (size_t)h->p.n * h->p.n, off = (size_t)env * nn;
    if (vx) CFDCHK(hipMemcpyAsync(vx, h->planes + off, nn * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (vy) CFDCHK(hipMemcpyAsync(vy, h->planes + h->plane + off, nn * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CFDCHK(hipStreamSynchronize(h->stream));
    return SF_OK;
}
