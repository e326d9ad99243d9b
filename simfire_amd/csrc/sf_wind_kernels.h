// Wind changes during an episode (sf_set_wind, sf_set_wind_schedule): the R tables of a list of environments
// rebuilt from new wind between two step launches.  The reference reads self.U / self.U_dir at every update()
// (simfire/game/managers/fire.py:365, 490-494): a caller who assigns new arrays between two updates gets a wind shift.
// Part of the single translation unit simfire_hip.hip.  Only phi_w depends on the wind (rothermel.py:104-111), so everything else of
// sfdev::CellTerms and the eight projected slopes are kept per cell in a cache plane (k_wind_terms) and k_wind_rtable makes the
// table from cache + wind.  The arithmetic is that of sfdev::cell_terms / sfdev::ros_dir operation for operation (the library is
// built with -ffp-contract=off), so a table is bit-identical to what sf_set_layers_env builds from the same planes.
#pragma once
#include "sf_common.h"
#include "sf_aux_kernels.h"

namespace {

constexpr int kWindThreads = 256;
constexpr int kWindPlanes = 16;      // float planes [H * W] per table of the cache: 64 bytes per cell (15 used)
// cache planes: 0 burnable (0 / 1), 1 IRxi, 2 den, 3 c, 4 b, 5 ratio_e, 6 Bs, 7 .. 14 the projected slope s of ros_dir per direction

// A schedule of uniform winds for one environment (sf_set_wind_schedule) and the segment its table was last built for.
struct WindSched {
    int32_t K;          // segments set (0: no schedule)
    int32_t seg;        // the segment the table stands for, -1 = unknown
    sf_wind_seg rows[SF_WIND_MAX_SEGS];
};

// What a cell contributes to its eight rates apart from the wind.
struct WindTerms {
    bool burnable;
    float IRxi, den, c, b, ratio_e, Bs;
    float s[8];
};

// cell (x, y) of the layer planes L ([7][H * W]) -> its terms: cell_terms with the slope of slope_at rounded to float32, as k_gen_rtable
__device__ inline WindTerms wind_terms_at(int H, int W, const double *L, double ps, float h, float S_T, float S_e, float p_p, float M_f,
                                          const Thetas &th, int x, int y)
{
    const long long n = (long long)H * W, i = (long long)y * W + x;
    double mag, dir;
    slope_at(H, W, L + 4 * n, ps, x, y, mag, dir);
    const sfdev::CellTerms t = sfdev::cell_terms((float)L[i], (float)L[n + i], (float)L[2 * n + i], (float)L[3 * n + i], h, S_T, S_e, p_p,
                                                 M_f, 0.0f, 0.0f, (float)mag, (float)dir);
    WindTerms w;
    w.burnable = t.burnable;
    w.IRxi = t.IRxi; w.den = t.den; w.c = t.c; w.b = t.b; w.ratio_e = t.ratio_e; w.Bs = t.Bs;
#pragma unroll
    for (int k = 0; k < 8; ++k) w.s[k] = (-t.slope_mag) * sfdev::cs(t.slope_dir + th.v[k]);      // rothermel.py:117
    return w;
}

// ros_dir from the wind-independent terms, the wind's along-travel component Ua (rothermel.py:105-110) and direction k
__device__ __forceinline__ double wind_ros(const WindTerms &w, float Ua, int k)
{
    if (!w.burnable) return 0.0;                                            // rothermel.py:127-130
    const float p = (Ua == 0.0f && w.b > 0.0f) ? 0.0f : sfdev::pw(Ua, w.b); // pow(0, b > 0) is exactly 0
    const float phi_w = (w.c * p) * w.ratio_e;                              // :111
    const float s = w.s[k];
    const double sign = (s > 0.0f) ? 1.0 : -1.0;                            // :118
    const double phi_s = ((double)w.Bs * sign) * (double)(s * s);           // :119
    const double num = (double)w.IRxi * ((double)(1.0f + phi_w) + phi_s);
    const double R = num / (double)w.den;                                   // :128
    return R > 0.0 ? R : 0.0;                                               // :134
}

// The cache planes of tables list[z] (list != null) or t0 + z, z = blockIdx.z; workgroup (column block, row, table).
__global__ __launch_bounds__(kWindThreads) void k_wind_terms(int H, int W, const double *lay, const int32_t *list, int t0, double ps, float h,
                                                            float S_T, float S_e, float p_p, float M_f, Thetas th, float *cache)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int t = list ? list[blockIdx.z] : t0 + (int)blockIdx.z;
    const long long n = (long long)H * W, i = (long long)y * W + x;
    const WindTerms w = wind_terms_at(H, W, lay + (long long)t * 7 * n, ps, h, S_T, S_e, p_p, M_f, th, x, y);
    float *c = cache + (long long)t * kWindPlanes * n + i;
    c[0] = w.burnable ? 1.0f : 0.0f;
    c[n] = w.IRxi; c[2 * n] = w.den; c[3 * n] = w.c; c[4 * n] = w.b; c[5 * n] = w.ratio_e; c[6 * n] = w.Bs;
#pragma unroll
    for (int k = 0; k < 8; ++k) c[(7 + k) * n] = w.s[k];
}

struct WindArgs {
    int H, W, P;
    double *lay;                 // [tables][7][H * W]: planes 5 and 6 of a listed table are written
    const float *cache;          // [tables][kWindPlanes][H * W] (k_wind_rtable<false>: not read)
    double *rt, *rtc;            // direction-major tables; the cell-major copies or null
    long long tab_stride;        // elements between two tables
    const int32_t *list;         // listed tables (device memory)
    const uint32_t *count_dev;   // their number in device memory, or null: count
    int count;
    const double *U, *U_dir;     // uniform: [listed]; field: [listed][H * W]
    int field;
    double ps;
    float h, S_T, S_e, p_p, M_f;
    Thetas th;
};

// Cache (or, CACHED = false, the layers) + wind -> the tables of the listed environments, both layouts, and their wind planes.  A
// grid-stride loop over (listed table, row, block of kWindThreads columns); an empty list costs a workgroup one load.
template <bool CACHED>
__global__ __launch_bounds__(kWindThreads) void k_wind_rtable(WindArgs a)
{
    __shared__ float ua_env[8];
    const int cb = (a.P + kWindThreads - 1) / kWindThreads;
    const long long per_tab = (long long)a.H * cb;
    const long long total = (long long)(a.count_dev ? (int)*a.count_dev : a.count) * per_tab;
    const long long n = (long long)a.H * a.W, plane = (long long)a.H * a.P;
    long long last = -1;
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long li = w / per_tab;
        const int r = (int)(w - li * per_tab);
        const int y = r / cb, x = (r - y * cb) * kWindThreads + (int)threadIdx.x;
        const int t = a.list[li];
        if (!a.field && li != last) {         // the eight cs(omega - theta) once per table (every lane of the workgroup takes this branch or none)
            __syncthreads();
            if (threadIdx.x < 8) {
                const float U = (float)a.U[li];
                const float omega = (90.0f - (float)a.U_dir[li]) * 0.017453292519943295f;      // rothermel.py:104
                ua_env[threadIdx.x] = fmaxf(U * sfdev::cs(omega - a.th.v[threadIdx.x]), 0.0f);
            }
            __syncthreads();
            last = li;
        }
        if (x >= a.P) continue;
        double *out = a.rt + (long long)t * a.tab_stride;
        const long long o = (long long)y * a.P + x;
        double R[8];
        if (x >= a.W) {
#pragma unroll
            for (int k = 0; k < 8; ++k) R[k] = 0.0;
        } else {
            const long long i = (long long)y * a.W + x;
            double *L = a.lay + (long long)t * 7 * n;
            WindTerms wt;
            if (CACHED) {
                const float *c = a.cache + (long long)t * kWindPlanes * n + i;
                wt.burnable = c[0] != 0.0f;
                wt.IRxi = c[n]; wt.den = c[2 * n]; wt.c = c[3 * n]; wt.b = c[4 * n]; wt.ratio_e = c[5 * n]; wt.Bs = c[6 * n];
#pragma unroll
                for (int k = 0; k < 8; ++k) wt.s[k] = c[(7 + k) * n];
            } else {
                wt = wind_terms_at(a.H, a.W, L, a.ps, a.h, a.S_T, a.S_e, a.p_p, a.M_f, a.th, x, y);
            }
            const double Ud = a.field ? a.U[li * n + i] : a.U[li], Dd = a.field ? a.U_dir[li * n + i] : a.U_dir[li];
            L[5 * n + i] = Ud;
            L[6 * n + i] = Dd;
            if (a.field) {
                const float U = (float)Ud;
                const float omega = (90.0f - (float)Dd) * 0.017453292519943295f;
#pragma unroll
                for (int k = 0; k < 8; ++k) R[k] = wind_ros(wt, wt.burnable ? fmaxf(U * sfdev::cs(omega - a.th.v[k]), 0.0f) : 0.0f, k);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) R[k] = wind_ros(wt, ua_env[k], k);
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k * plane + o] = R[k];
        if (a.rtc) {
            double2 *dst = reinterpret_cast<double2 *>(a.rtc + (long long)t * a.tab_stride + o * 8);
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[k] = make_double2(R[2 * k], R[2 * k + 1]);
        }
    }
}

// sf_set_wind_schedule: rows[i][K] become environment list[i]'s schedule (K = 0: none), its segment unknown
__global__ void k_wind_sched_set(int n, const int32_t *list, int K, const sf_wind_seg *rows, WindSched *sched)
{
    const int i = blockIdx.x, k = threadIdx.x;
    if (i >= n) return;
    WindSched &d = sched[list[i]];
    if (k < K) d.rows[k] = rows[(long long)i * K + k];
    if (k == 0) { d.K = K; d.seg = -1; }
}

// segment unknown for the listed environments (sf_load_state)
__global__ void k_wind_sched_forget(int n, const int32_t *list, WindSched *sched)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sched[list[i]].seg = -1;
}

// In front of a stepping call while a schedule is set: every scheduled environment whose update count - as the next launch will see
// it (entering_state, the way k_mitigate_clear resolves it) - lies in another segment than the one its table stands for is appended
// to the due list with that segment's wind.  *cnt is zero when the kernel starts.
__global__ void k_wind_due(Geo g, const EnvState *commit, const EnvState *tmp, const uint32_t *flags, int launch, int from_commit,
                           WindSched *sched, uint32_t *cnt, int32_t *due, double *U, double *U_dir)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= g.E) return;
    WindSched &d = sched[e];
    const int K = d.K;
    if (K == 0) return;
    const int steps = entering_state(commit, tmp, flags, launch, from_commit, e, g).steps;
    int seg = 0;
    for (int k = 1; k < K; ++k) if (d.rows[k].first_update <= steps) seg = k;
    if (seg == d.seg) return;
    d.seg = seg;
    const uint32_t at = atomicAdd(cnt, 1u);
    due[at] = e;
    U[at] = d.rows[seg].U;
    U_dir[at] = d.rows[seg].U_dir;
}

}  // namespace
