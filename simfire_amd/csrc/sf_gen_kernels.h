// Seeded worlds drawn on the device (sf_generate_layers): perlin topography, chaparral fuel scalars and perlin
// wind written straight into the layer planes of a list of environments, then their R tables rebuilt in one batched launch.
// Replaces, per environment, FireSimulation.set_seeds + reset's rebuild of the seeded layers (simfire/sim/simulation.py:713-759,
// 202-214): elevation_functions.py:75-122, terrain.py:29-114 (its scalars come from the host), perlin_wind.py:69-98 + config.py:892-944.
// Part of the single translation unit simfire_hip.hip.  float64 in the order of the host oracles (simfire_amd/workloads.py:
// simplex2, fractal_simplex, perlin_elevation, simplex_field); the library is built with -ffp-contract=off, which that order relies on.
#pragma once
#include "sf_common.h"
#include "sf_aux_kernels.h"

namespace {

constexpr int kGenThreads = 256;
constexpr int kGenMaxOctaves = 16;
constexpr int kGenChunk = 65535;         // listed environments per launch (grid y / z limit)

// Ken Perlin's permutation, the table of workloads._PERM
__constant__ uint8_t kGenPerm[256] = {
    151, 160, 137, 91, 90, 15, 131, 13, 201, 95, 96, 53, 194, 233, 7, 225, 140, 36, 103, 30, 69, 142, 8, 99, 37, 240, 21,
    10, 23, 190, 6, 148, 247, 120, 234, 75, 0, 26, 197, 62, 94, 252, 219, 203, 117, 35, 11, 32, 57, 177, 33, 88, 237, 149,
    56, 87, 174, 20, 125, 136, 171, 168, 68, 175, 74, 165, 71, 134, 139, 48, 27, 166, 77, 146, 158, 231, 83, 111, 229,
    122, 60, 211, 133, 230, 220, 105, 92, 41, 55, 46, 245, 40, 244, 102, 143, 54, 65, 25, 63, 161, 1, 216, 80, 73, 209, 76,
    132, 187, 208, 89, 18, 169, 200, 196, 135, 130, 116, 188, 159, 86, 164, 100, 109, 198, 173, 186, 3, 64, 52, 217, 226,
    250, 124, 123, 5, 202, 38, 147, 118, 126, 255, 82, 85, 212, 207, 206, 59, 227, 47, 16, 58, 17, 182, 189, 28, 42, 223,
    183, 170, 213, 119, 248, 152, 2, 44, 154, 163, 70, 221, 153, 101, 155, 167, 43, 172, 9, 129, 22, 39, 253, 19, 98, 108,
    110, 79, 113, 224, 232, 178, 185, 112, 104, 218, 246, 97, 228, 251, 34, 242, 193, 238, 210, 144, 12, 191, 179, 162,
    241, 81, 51, 145, 235, 249, 14, 239, 107, 49, 192, 214, 31, 181, 199, 106, 157, 184, 84, 204, 176, 115, 121, 50, 45,
    127, 4, 150, 254, 138, 236, 205, 93, 222, 114, 67, 29, 24, 72, 243, 141, 128, 195, 78, 66, 215, 61, 156, 180};

// F2 = 0.5 * (sqrt(3) - 1), G2 = (3 - sqrt(3)) / 6 as NumPy rounds them
constexpr double kGenF2 = 0x1.76cf5d0b09954p-2, kGenG2 = 0x1.b0cb174df99c8p-3;

// one corner of simplex2: tt^4 * (g . (xc, yc)) where tt > 0, gradient _GRAD2[gi % 12] (components +-1 / 0: the dot product is
// formed exactly as NumPy forms it).  tt^4 is (tt * tt) * (tt * tt), where NumPy calls pow(tt, 4): the float64 value can differ in
// the last bit; the float32 planes this feeds are the same
__device__ inline double gen_corner(double xc, double yc, int gi)
{
    const double tt = 0.5 - xc * xc - yc * yc;
    if (!(tt > 0.0)) return 0.0;
    const int k = gi % 12;
    const double gx = k < 8 ? ((k & 1) ? -1.0 : 1.0) : 0.0;
    const double gy = k < 4 ? ((k & 2) ? -1.0 : 1.0) : (k < 8 ? 0.0 : ((k & 1) ? -1.0 : 1.0));
    const double t2 = tt * tt;
    return (t2 * t2) * (gx * xc + gy * yc);
}

// workloads.simplex2 at one point; perm = the table twice (512 entries, LDS)
__device__ inline double gen_simplex2(double x, double y, long long base, const uint8_t *perm)
{
    const double s = (x + y) * kGenF2;
    const double i = floor(x + s), j = floor(y + s);
    const double t = (i + j) * kGenG2;
    const double x0 = x - (i - t), y0 = y - (j - t);
    const int i1 = x0 > y0 ? 1 : 0, j1 = 1 - i1;
    const double x1 = x0 - (double)i1 + kGenG2, y1 = y0 - (double)j1 + kGenG2;
    const double x2 = x0 - 1.0 + 2.0 * kGenG2, y2 = y0 - 1.0 + 2.0 * kGenG2;
    const int ii = (int)(((long long)i + base) & 255), jj = (int)(((long long)j + base) & 255);     // 64-bit, like NumPy's int64
    const double n = gen_corner(x0, y0, perm[ii + perm[jj]]) + gen_corner(x1, y1, perm[ii + i1 + perm[jj + j1]]) +
                     gen_corner(x2, y2, perm[ii + 1 + perm[jj + 1]]);
    return 70.0 * n;
}

// workloads.fractal_simplex at cell (x, y)
__device__ inline double gen_fractal(double x, double y, const sf_noise &p, const uint8_t *perm)
{
    x = x / p.scale;
    y = y / p.scale;
    double total = 0.0, amp = 1.0, freq = 1.0, norm = 0.0;
    for (int o = 0; o < p.octaves; ++o) {
        total += gen_simplex2(x * freq, y * freq, (long long)p.seed, perm) * amp;
        norm += amp;
        freq *= p.lacunarity;
        amp *= p.persistence;
    }
    return total / norm;
}

// Workgroup (cell block, listed environment y0 + blockIdx.y, plane group blockIdx.z: 0 elevation, 1 fuel, 2 wind speed, 3 wind
// direction).  A group the descriptor does not name returns at once (uniformly), so its planes keep their bytes.
__global__ __launch_bounds__(kGenThreads) void k_gen_planes(int H, int W, double *lay, const int32_t *envs, const sf_layer_gen *gens, int y0)
{
    __shared__ uint8_t perm[512];
    const int li = y0 + (int)blockIdx.y, grp = (int)blockIdx.z;
    const sf_layer_gen &d = gens[li];
    const long long n = (long long)H * W;
    double *tab = lay + (long long)envs[li] * 7 * n;
    const long long c = (long long)blockIdx.x * kGenThreads + threadIdx.x;
    if (grp == 1) {
        if (d.fuel != SF_GEN_CONSTANT || c >= n) return;
        for (int k = 0; k < 4; ++k) tab[k * n + c] = d.fuel_values[k];
        return;
    }
    const sf_noise p = grp == 0 ? d.elevation : (grp == 2 ? d.wind_speed : d.wind_direction);
    if (p.kind == SF_GEN_NONE) return;
    double *out = tab + (grp == 0 ? 4 : grp + 3) * n;
    if (p.kind == SF_GEN_CONSTANT) {
        if (c < n) out[c] = p.lo;
        return;
    }
    for (int k = threadIdx.x; k < 512; k += kGenThreads) perm[k] = kGenPerm[k & 255];
    __syncthreads();
    if (c >= n) return;
    const double f = gen_fractal((double)(c % W), (double)(c / W), p, perm);
    if (grp == 0) {                 // perlin_elevation: snoise2's float32, then the range map in float64
        const double z = (double)(float)f;
        out[c] = ((z + 1.0) / 2.0) * (p.hi - p.lo) + p.lo;
    } else {                        // simplex_field: the range map in float64, then float32, widened
        out[c] = (double)(float)((((f + 1.0) * (p.hi - p.lo)) / 2.0) + p.lo);
    }
}

// k_slopes + k_rtable for the listed environments in one launch: workgroup (column block, row, listed environment z0 + blockIdx.z);
// the slopes come from the same slope_at as k_slopes and go through the same float32 rounding into cell_terms, so every table is
// bit-identical to what sf_set_layers_env makes of the same planes.  No slope scratch plane.
__global__ __launch_bounds__(kGenThreads) void k_gen_rtable(int H, int W, int P, const double *lay, const int32_t *envs, int z0, double ps,
                                                           float h, float S_T, float S_e, float p_p, float M_f, Thetas th, double *rt,
                                                           long long tab_stride)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= P) return;
    const int e = envs[z0 + (int)blockIdx.z];
    const long long n = (long long)H * W;
    const double *L = lay + (long long)e * 7 * n;
    double *out = rt + (long long)e * tab_stride;
    const long long o = (long long)y * P + x, plane = (long long)H * P;
    if (x >= W) {
        for (int k = 0; k < 8; ++k) out[k * plane + o] = 0.0;
        return;
    }
    const long long i = (long long)y * W + x;
    double mag, dir;
    slope_at(H, W, L + 4 * n, ps, x, y, mag, dir);
    const sfdev::CellTerms t = sfdev::cell_terms((float)L[i], (float)L[n + i], (float)L[2 * n + i], (float)L[3 * n + i], h, S_T, S_e, p_p,
                                                 M_f, (float)L[5 * n + i], (float)L[6 * n + i], (float)mag, (float)dir);
    for (int k = 0; k < 8; ++k) out[k * plane + o] = sfdev::ros_dir(t, th.v[k]);
}

}  // namespace
