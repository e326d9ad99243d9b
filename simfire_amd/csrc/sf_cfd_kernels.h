// CFD wind field: the reference's stable-fluids velocity solver, batched over environments, one workgroup per environment.
//
// Replaces (reference mitrefireline/simfire v2.0.1):
//   Fluid.step (velocity part)          simfire/world/wind_mechanics/cfd_wind.py:49-60
//   set_bnd / lin_solve / diffuse        cfd_wind.py:104-165, 168-192, 195-208
//   project / advect                     cfd_wind.py:211-247, 250-298
//   WindControllerCFD.iterate_wind_step  simfire/world/wind_mechanics/wind_controller.py:156-170
//
// Every value is the reference's f64 expression in the reference's evaluation order (no FMA contraction: the library is
// built with -ffp-contract=off), so the planes are bit-identical to the Python loops.  The density / `s` planes never feed
// the velocity and are not computed.
//
// Structure ("CFD wind"): the four planes Vx, Vy, Vx0, Vy0 live in device memory, [E][N][N] f64 each, the terrain
// mask [E][N][N] u8.  A workgroup of 1024 threads owns one environment for a chunk of Fluid.step()s.
//   * lin_solve's in-place Gauss-Seidel pass (j outer, i inner) runs as a wavefront: the lane of row i computes cell (i, j) at
//     step s = i + j.  (i, j-1) is the lane's own previous result, (i-1, j) the previous step's result of the lane above (a
//     shuffle inside a wave; across waves an LDS ring with one progress word per producer wave, polled with s_sleep), and
//     (i+1, j), (i, j+1) are the values from before the pass, read from memory a few steps ahead of use.  More interior rows
//     than lanes: strips of 1024 rows one after another (a strip needs only the finished last row of the strip before it).
//   * The other passes (set_bnd's edges / corners / terrain parity, project's divergence and gradient, advect's gather, the
//     inflow) are workgroup-wide loops with __syncthreads() between them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int CFD_THREADS = 1024;
constexpr int CFD_WAVES = CFD_THREADS / 64;
constexpr int CFD_RING = 256;           // steps a producer wave may run ahead of its consumer (ring slots per wave)
constexpr int CFD_MAX_N = 4096;         // LDS: ring (64 KiB) + the row above a strip (N x 2 f64)
constexpr int CFD_SPIN_LIMIT = 1 << 22; // bound of one wavefront wait (~64 clocks per poll): a wait this long is an error

struct CfdArgs {
    double *vx, *vy, *vx0, *vy0;  // [E][N][N]
    const uint8_t *mask;          // [E][N][N], 1 = terrain above the average elevation
    int *err;                     // set to 1 when a wavefront wait ran out (the result is then not the reference's)
    int n, itr, direction, n_steps, inflow_every, k0;
    double a_diff, cr_diff, cr_proj, dtx, speed;
};

inline size_t cfd_lds_bytes(int n)
{
    return (size_t)CFD_WAVES * CFD_RING * 2 * sizeof(double) + (size_t)n * 2 * sizeof(double) + 2 * CFD_WAVES * sizeof(int);
}

struct CfdLds {
    double *ring;   // [CFD_WAVES][CFD_RING][NCH]: lane 63's result of every step
    double *above;  // [N][NCH]: the row above the current strip, final for this pass
    int *prog;      // [CFD_WAVES]: last step a wave has finished (volatile access)
    int *abort;     // [1]: a wait ran out - no more waiting in this launch
};

__device__ inline int lds_ld(const int *p) { return *(const volatile int *)p; }
__device__ inline void lds_st(int *p, int v) { *(volatile int *)p = v; }

// set_bnd(b, x) for NCH planes at once (cfd_wind.py:104-165): edges, corners, then (b = 1, 2) the terrain step.  In the
// reference the terrain step is a sequential loop over rows and columns 2..N-3 that zeroes a mask cell and negates each
// non-mask neighbour on the b axis; a non-mask cell is never zeroed and a mask cell never negated, so the result is: mask
// cells in 2..N-3 -> 0.0, every other interior cell negated once per mask neighbour in 2..N-3 - order-free.
template <int NCH>
__device__ void cfd_set_bnd(double *const x[NCH], const int b[NCH], const uint8_t *mask, int N)
{
    const int tid = threadIdx.x;
    for (int t = tid; t < N - 2; t += CFD_THREADS) {
        const int k = t + 1;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            double *p = x[c];
            p[k * N + 0] = b[c] == 2 ? -p[k * N + 1] : p[k * N + 1];
            p[k * N + N - 1] = b[c] == 2 ? -p[k * N + N - 2] : p[k * N + N - 2];
            p[0 * N + k] = b[c] == 1 ? -p[1 * N + k] : p[1 * N + k];
            p[(N - 1) * N + k] = b[c] == 1 ? -p[(N - 2) * N + k] : p[(N - 2) * N + k];
        }
    }
    __syncthreads();
    if (tid < NCH) {
        double *p = x[tid];
        p[0] = 0.5 * (p[1 * N + 0] + p[0 * N + 1]);
        p[N - 1] = 0.5 * (p[1 * N + N - 1] + p[0 * N + N - 2]);
        p[(N - 1) * N + 0] = 0.5 * (p[(N - 2) * N + 0] + p[(N - 1) * N + 1]);
        p[(N - 1) * N + N - 1] = 0.5 * (p[(N - 2) * N + N - 1] + p[(N - 1) * N + N - 2]);
    }
    __syncthreads();
    bool terrain = false;
#pragma unroll
    for (int c = 0; c < NCH; ++c) terrain |= b[c] != 0;
    if (!terrain) return;
    const int M = N - 2;
    auto in = [N](int r) { return r >= 2 && r <= N - 3; };
    for (int t = tid; t < M * M; t += CFD_THREADS) {
        const int i = 1 + t / M, j = 1 + t % M;
        const bool m = mask[i * N + j] != 0;
        if (m && !(in(i) && in(j))) continue;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (b[c] == 0) continue;
            double *p = x[c] + i * N + j;
            if (m) {
                *p = 0.0;
                continue;
            }
            int cnt = 0;
            if (b[c] == 2 && in(i))
                cnt = (in(j - 1) && mask[i * N + j - 1]) + (in(j + 1) && mask[i * N + j + 1]);
            if (b[c] == 1 && in(j))
                cnt = (in(i - 1) && mask[(i - 1) * N + j]) + (in(i + 1) && mask[(i + 1) * N + j]);
            if (cnt & 1) *p = -*p;
        }
    }
    __syncthreads();
}

// One in-place Gauss-Seidel pass of lin_solve (cfd_wind.py:176-191) over NCH independent chains, as a wavefront.
//   calc = (x0[i][j] + a*(((x[i+1][j] + x[i-1][j]) + x[i][j+1]) + x[i][j-1])) * cRecip;  a mask cell gets 0.0
// B steps are prefetched per lane (memory reads of the old right / lower neighbours and of x0) and per wave (the LDS values
// of the row above).
template <int NCH, int B>
__device__ void cfd_gs_pass(double *const x[NCH], const double *const x0[NCH], const uint8_t *mask, int N, double a, double cr,
                            CfdLds &L, int *err)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int rows = N - 2;
    for (int strip = 0; strip < rows; strip += CFD_THREADS) {
        const int srows = min(CFD_THREADS, rows - strip);
        const int nw = (srows + 63) >> 6;
        const int i = 1 + strip + tid;
        const bool row_ok = tid < srows;
        const int wrow0 = 1 + strip + (wave << 6);
        const int wlast = min(wrow0 + 63, strip + srows);
        const int sb = wrow0 + 1, se = wlast + N - 2;
        const int se_prev = wrow0 - 1 + N - 2;  // last step of the wave above (all its 64 rows are interior rows)
        for (int t = tid; t < N; t += CFD_THREADS)
#pragma unroll
            for (int c = 0; c < NCH; ++c) L.above[t * NCH + c] = x[c][strip * N + t];
        if (lane == 0) lds_st(&L.prog[wave], sb - 1);
        __syncthreads();
        if (wave < nw) {
            const int ir = row_ok ? i : 1;  // rows past the strip compute garbage from row 1 and store nothing
            double left[NCH], rt[B][NCH], dn[B][NCH], src[B][NCH];
            bool mk[B];
#pragma unroll
            for (int c = 0; c < NCH; ++c) left[c] = x[c][ir * N];
            auto fetch = [&](int k, int s) {
                const int j = s - i;
                const bool ok = row_ok && j >= 1 && j <= N - 2;
                const int jj = ok ? j : 1;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    rt[k][c] = ok ? x[c][ir * N + jj + 1] : 0.0;
                    dn[k][c] = ok ? x[c][(ir + 1) * N + jj] : 0.0;
                    src[k][c] = ok ? x0[c][ir * N + jj] : 0.0;
                }
                mk[k] = ok ? mask[ir * N + jj] != 0 : false;
            };
#pragma unroll
            for (int k = 0; k < B; ++k) fetch(k, sb + k);
            double *ring_out = L.ring + (size_t)wave * CFD_RING * NCH;
            const double *ring_in = L.ring + (size_t)(wave - 1) * CFD_RING * NCH;
            for (int s0 = sb; s0 <= se; s0 += B) {
                // wait: the wave above has finished the steps this block reads; the wave below has read the ring slots this
                // block overwrites
                if (!lds_ld(L.abort)) {
                    const int need_up = min(s0 + B - 2, se_prev);
                    const int need_dn = s0 + B - CFD_RING;
                    int spins = 0;
                    while ((wave > 0 && lds_ld(&L.prog[wave - 1]) < need_up) ||
                           (wave + 1 < nw && lds_ld(&L.prog[wave + 1]) < need_dn)) {
                        __builtin_amdgcn_s_sleep(1);
                        if (++spins > CFD_SPIN_LIMIT) {
                            lds_st(L.abort, 1);
                            *err = 1;
                            break;
                        }
                    }
                }
                __asm__ volatile("" ::: "memory");
                double upl[B][NCH];
#pragma unroll
                for (int k = 0; k < B; ++k) {
                    const int s = s0 + k;
                    int jl = s - wrow0;
                    jl = jl < 0 ? 0 : (jl > N - 1 ? N - 1 : jl);
#pragma unroll
                    for (int c = 0; c < NCH; ++c)
                        upl[k][c] = wave == 0 ? L.above[jl * NCH + c] : ring_in[((s - 1) & (CFD_RING - 1)) * NCH + c];
                }
#pragma unroll
                for (int k = 0; k < B; ++k) {
                    const int s = s0 + k;
                    const int j = s - i;
                    const bool active = row_ok && j >= 1 && j <= N - 2;
#pragma unroll
                    for (int c = 0; c < NCH; ++c) {
                        double up = __shfl_up(left[c], 1);
                        if (lane == 0) up = upl[k][c];
                        const double sum = ((dn[k][c] + up) + rt[k][c]) + left[c];
                        const double calc = (src[k][c] + a * sum) * cr;
                        const double v = mk[k] ? 0.0 : calc;
                        if (active) {
                            x[c][i * N + j] = v;
                            left[c] = v;
                        }
                        if (lane == 63) ring_out[(s & (CFD_RING - 1)) * NCH + c] = left[c];
                    }
                    fetch(k, s + B);
                }
                __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (lane == 0) lds_st(&L.prog[wave], s0 + B - 1);
            }
        }
        __syncthreads();
    }
}

template <int NCH>
__device__ void cfd_lin_solve(double *const x[NCH], const double *const x0[NCH], const int b[NCH], const uint8_t *mask, int N,
                              int itr, double a, double cr, CfdLds &L, int *err)
{
    for (int t = 0; t < itr; ++t) {
        cfd_gs_pass<NCH, 4 / NCH>(x, x0, mask, N, a, cr, L, err);
        cfd_set_bnd<NCH>(x, b, mask, N);
    }
}

// project(velocX, velocY, p, div), cfd_wind.py:211-247
__device__ void cfd_project(double *u, double *v, double *p, double *div, const uint8_t *mask, int N, int itr, double cr,
                            CfdLds &L, int *err)
{
    const int M = N - 2;
    const double Nd = (double)N;
    for (int t = threadIdx.x; t < M * M; t += CFD_THREADS) {
        const int i = 1 + t / M, j = 1 + t % M, q = i * N + j;
        div[q] = (-0.5 * (((u[q + N] - u[q - N]) + v[q + 1]) - v[q - 1])) / Nd;
        p[q] = 0.0;
    }
    __syncthreads();
    {
        double *const xs[2] = {div, p};
        const int bs[2] = {0, 0};
        cfd_set_bnd<2>(xs, bs, mask, N);
    }
    {
        double *const xs[1] = {p};
        const double *const x0s[1] = {div};
        const int bs[1] = {0};
        cfd_lin_solve<1>(xs, x0s, bs, mask, N, itr, 1.0, cr, L, err);
    }
    for (int t = threadIdx.x; t < M * M; t += CFD_THREADS) {
        const int i = 1 + t / M, j = 1 + t % M, q = i * N + j;
        u[q] = u[q] - (0.5 * (p[q + N] - p[q - N])) * Nd;
        v[q] = v[q] - (0.5 * (p[q + 1] - p[q - 1])) * Nd;
    }
    __syncthreads();
    double *const xs[2] = {u, v};
    const int bs[2] = {1, 2};
    cfd_set_bnd<2>(xs, bs, mask, N);
}

// advect(1, Vx, Vx0, Vx0, Vy0) and advect(2, Vy, Vy0, Vx0, Vy0) in one gather pass, cfd_wind.py:250-298.  Only the first half
// of the reference's bilinear blend survives: line 296 ends the assignment `d[i][j] = s0 * (...)`, and line 297's
// `+s1 * (...)` is a separate expression statement whose value is discarded.  So d = s0*(t0*d0[i0][j0] + t1*d0[i0][j1]).
__device__ void cfd_advect(double *vx, double *vy, const double *vx0, const double *vy0, const uint8_t *mask, int N, double dtx)
{
    const int M = N - 2;
    const double hi = (double)M + 0.5;
    for (int t = threadIdx.x; t < M * M; t += CFD_THREADS) {
        const int i = 1 + t / M, j = 1 + t % M, q = i * N + j;
        double x = (double)i - dtx * vx0[q];
        double y = (double)j - dtx * vy0[q];
        if (x < 0.5) x = 0.5;
        if (x > hi) x = hi;
        if (y < 0.5) y = 0.5;
        if (y > hi) y = hi;
        const double fi = floor(x), fj = floor(y);
        const double s1 = x - fi, s0 = 1.0 - s1, t1 = y - fj, t0 = 1.0 - t1;
        int i0 = (int)fi, j0 = (int)fj;
        // (a NaN velocity would make the reference raise in math.floor; clamp so the gather stays inside the plane)
        i0 = i0 < 0 ? 0 : (i0 > N - 2 ? N - 2 : i0);
        j0 = j0 < 0 ? 0 : (j0 > N - 2 ? N - 2 : j0);
        const int r = i0 * N + j0;
        vx[q] = s0 * (t0 * vx0[r] + t1 * vx0[r + 1]);
        vy[q] = s0 * (t0 * vy0[r] + t1 * vy0[r + 1]);
    }
    __syncthreads();
    double *const xs[2] = {vx, vy};
    const int bs[2] = {1, 2};
    cfd_set_bnd<2>(xs, bs, mask, N);
}

// n_steps Fluid.step()s of one environment per workgroup; step k (k0 + k counted within the host call) is preceded by the
// inflow of iterate_wind_step when inflow_every > 0 && (k0 + k) % inflow_every == 0.
__global__ void __launch_bounds__(CFD_THREADS) k_cfd(CfdArgs A)
{
    extern __shared__ double cfd_lds[];
    const int N = A.n;
    const size_t off = (size_t)blockIdx.x * N * N;
    double *Vx = A.vx + off, *Vy = A.vy + off, *Vx0 = A.vx0 + off, *Vy0 = A.vy0 + off;
    const uint8_t *mask = A.mask + off;
    CfdLds L;
    L.ring = cfd_lds;
    L.above = cfd_lds + (size_t)CFD_WAVES * CFD_RING * 2;
    L.prog = reinterpret_cast<int *>(L.above + (size_t)N * 2);
    L.abort = L.prog + CFD_WAVES;
    if (threadIdx.x == 0) lds_st(L.abort, 0);
    __syncthreads();
    for (int k = 0; k < A.n_steps; ++k) {
        if (A.inflow_every > 0 && (A.k0 + k) % A.inflow_every == 0) {
            // addVelocity(x, y, ax, ay) for v in 0..N-1 (wind_controller.py:156-170); the `+= 0` of the other component turns
            // -0.0 into +0.0 and is kept.  East writes a boundary cell that diffuse overwrites before anything reads it.
            for (int v = threadIdx.x; v < N; v += CFD_THREADS) {
                int q;
                double ax, ay;
                switch (A.direction) {
                case 0: q = v * N + 1; ax = 0.0; ay = A.speed; break;         // north
                case 1: q = (N - 1) * N + v; ax = -A.speed; ay = 0.0; break;  // east
                case 2: q = 1 * N + v; ax = -A.speed; ay = 0.0; break;        // south
                default: q = 1 * N + v; ax = A.speed; ay = 0.0; break;        // west
                }
                Vx[q] += ax;
                Vy[q] += ay;
            }
            __syncthreads();
        }
        {   // diffuse(1, Vx0, Vx) and diffuse(2, Vy0, Vy): independent solves, two chains of one sweep
            double *const xs[2] = {Vx0, Vy0};
            const double *const x0s[2] = {Vx, Vy};
            const int bs[2] = {1, 2};
            cfd_lin_solve<2>(xs, x0s, bs, mask, N, A.itr, A.a_diff, A.cr_diff, L, A.err);
        }
        cfd_project(Vx0, Vy0, Vx, Vy, mask, N, A.itr, A.cr_proj, L, A.err);
        cfd_advect(Vx, Vy, Vx0, Vy0, mask, N, A.dtx);
        cfd_project(Vx, Vy, Vx0, Vy0, mask, N, A.itr, A.cr_proj, L, A.err);
    }
}

}  // namespace
