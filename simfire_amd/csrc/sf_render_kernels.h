// Frames of environments (sf_render): what the reference's screen shows - the terrain image with the burned
// paint, the fire / line sprites and the agents on top (simfire/game/game.py:117-131, sprites.py:20-203, layers.py:744-768) - one
// pixel per cell, downscaled by an integer factor, as uint8 RGB frames in caller-owned device memory.
// Part of the single translation unit simfire_hip.hip.  k_render reads whichever cell plane is current (or the history ring) and
// writes nothing but `out`.
#pragma once
#include "sf_common.h"

namespace {

constexpr int kRdThreads = 256;
constexpr int kRdMaxLevels = 32;         // contour levels kept per table (MaxNLocator(8) yields at most ~10 inside the range)
constexpr uint8_t kRdAgent = 8;          // staged-byte flag: a winning agent stands on the cell
constexpr int kRdFbfmColours = 21;       // FuelModelRGB13 entries (enums.py:200-222)
// FuelModelRGB13 (simfire/enums.py:200-222): the FBFM13 codes with a colour and the colour in [0, 1] per channel
constexpr int32_t kRdFbfmCodes[kRdFbfmColours] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 91, 92, 93, 98, 99, -32768, -9999, 32767};
constexpr double kRdFbfmRgb[kRdFbfmColours][3] = {
    {1.0, 1.0, 0.745098039}, {1.0, 1.0, 0.0}, {0.901960784, 0.77254902, 0.043137255}, {1.0, 0.82745098, 0.498039216},
    {1.0, 0.666666667, 0.4}, {0.803921569, 0.666666667, 0.4}, {0.537254902, 0.439215686, 0.266666667}, {0.82745098, 1.0, 0.745098039},
    {0.439215686, 0.658823529, 0.0}, {0.149019608, 0.450980392, 0.0}, {0.909803922, 0.745098039, 1.0}, {0.478431373, 0.556862745, 0.960784314},
    {0.77254902, 0.0, 1.0}, {0.517647, 0.0, 0.541176}, {0.623529, 0.631373, 0.941176}, {0.913725, 0.45098, 1.0}, {0.0, 0.0, 1.0},
    {0.74902, 0.74902, 0.74902}, {1.0, 1.0, 1.0}, {1.0, 1.0, 1.0}, {1.0, 1.0, 1.0}};

// One background word per cell: R | G << 8 | B << 16 | contour << 24 (the fuel colour for background "fuel"; bit 24: a contour pixel)
struct RenderBgArgs {
    int H, W;
    const double *lay;          // dense layers [tables][7][H * W]: w_0 delta M_x sigma elevation U U_dir
    long long lay_tab;          // doubles between two tables' layers
    const uint8_t *fuel_ix;     // FBFM tables: [tables][H * W] index into fbfm_rgb (255: a code without a colour), else unused
    const int32_t *tabs;        // [n] tables to build
    const int32_t *fbfm;        // [n] 1: table tabs[i] holds FBFM-coded fuel
    double *mm;                 // [n][2] min / max of the elevation plane (k_render_minmax)
    uint32_t *bg;               // [tables][H * W]
    uint32_t base;              // terrain_rgb (R | G << 8 | B << 16): the texture colour the fuel colour is blended from
    uint32_t fbfm_rgb[kRdFbfmColours];
};

// Python's / NumPy's float divmod (floor division; the remainder takes the sign of b), as matplotlib's ticker uses it
__device__ double rd_divmod(double a, double b, double *mod_out)
{
    double mod = fmod(a, b);
    double div = (a - mod) / b;
    if (mod != 0.0) {
        if ((b < 0.0) != (mod < 0.0)) { mod += b; div -= 1.0; }
    } else {
        mod = copysign(0.0, b);
    }
    double fd;
    if (div != 0.0) {
        fd = floor(div);
        if (div - fd > 0.5) fd += 1.0;
    } else {
        fd = copysign(0.0, a / b);
    }
    *mod_out = mod;
    return fd;
}

// 10 ** k for an integral k: exact products up to 1e22, and 1 / 10 ** -k below 1 (the correctly rounded quotient)
__device__ double rd_pow10(double k)
{
    const int a = (int)fabs(k);
    double p = 1.0;
    for (int i = 0; i < a; ++i) p *= 10.0;
    return k < 0.0 ? 1.0 / p : p;
}

// MaxNLocator's extended staircase of its default steps [1, 1.5, 2, 2.5, 3, 4, 5, 6, 8, 10] (ticker.py _staircase: 0.1 * steps[:-1],
// steps, 10 * steps[1]), entry i (a switch, not an array: no scratch)
__device__ double rd_step(int i)
{
#pragma clang fp contract(off)
    double v;
    switch (i < 9 ? i : (i < 19 ? i - 9 : 1)) {
    case 0: v = 1.0; break;
    case 1: v = 1.5; break;
    case 2: v = 2.0; break;
    case 3: v = 2.5; break;
    case 4: v = 3.0; break;
    case 5: v = 4.0; break;
    case 6: v = 5.0; break;
    case 7: v = 6.0; break;
    case 8: v = 8.0; break;
    default: v = 10.0; break;
    }
    return i < 9 ? 0.1 * v : (i < 19 ? v : 10.0 * v);
}

// The contour levels of ax.contour(z) with matplotlib's automatic choice (contour.py _autolev: MaxNLocator(7 + 1, min_n_ticks=1)
// .tick_values(zmin, zmax); ticker.py nonsingular / scale_range / _Edge_integer / _raw_ticks), in its f64 order of operations, trimmed
// to the levels strictly inside (zmin, zmax) - [zmin] if none is.  tests/_render_oracle.py restates it in Python.
__device__ int rd_levels(double zmin, double zmax, double *lev)
{
#pragma clang fp contract(off)
    const double expander = 1e-13, tiny = 1e-14;
    double vmin = zmin, vmax = zmax;
    if (!isfinite(vmin) || !isfinite(vmax)) {
        vmin = -expander; vmax = expander;
    } else {
        const double mabs = fmax(fabs(vmin), fabs(vmax));
        if (mabs < (1e6 / tiny) * 2.2250738585072014e-308) {
            vmin = -expander; vmax = expander;
        } else if (vmax - vmin <= mabs * tiny) {
            if (vmax == 0.0 && vmin == 0.0) { vmin = -expander; vmax = expander; }
            else { vmin -= expander * fabs(vmin); vmax += expander * fabs(vmax); }
        }
    }
    const double nbins = 8.0;
    const double dv = fabs(vmax - vmin), meanv = (vmax + vmin) / 2.0;
    const double offset = fabs(meanv) / dv < 100.0 ? 0.0 : copysign(rd_pow10(floor(log10(fabs(meanv)))), meanv);
    const double scale = rd_pow10(floor(log10(dv / nbins)));
    const double _vmin = vmin - offset, _vmax = vmax - offset;
    const double raw_step = (_vmax - _vmin) / nbins;
    int istep = 19;
    for (int i = 0; i < 20; ++i)
        if (rd_step(i) * scale >= raw_step) { istep = i; break; }
    double step = rd_step(istep) * scale, best = 0.0, low = 0.0, high = -1.0;
    for (int i = istep; i >= 0; --i) {
        step = rd_step(i) * scale;
        double m;
        best = rd_divmod(_vmin, step, &m) * step;
        double tol = 1e-10;
        if (fabs(offset) > 0.0) {
            const double digits = log10(fabs(offset) / step);
            tol = fmin(0.4999, fmax(1e-10, pow(10.0, digits - 12.0)));
        }
        low = rd_divmod(_vmin - best, step, &m);
        if (fabs(m / step - 1.0) < tol) low += 1.0;
        high = rd_divmod(_vmax - best, step, &m);
        if (!(fabs(m / step - 0.0) < tol)) high += 1.0;
        int nt = 0;
        for (double k = low; k <= high && k <= low + 64.0; k += 1.0) {
            const double t = k * step + best;
            nt += t <= _vmax && t >= _vmin;
        }
        if (nt >= 1) break;
    }
    int n = 0;
    for (double k = low; k <= high && k <= low + 64.0; k += 1.0) {
        const double L = (k * step + best) + offset;
        if (L > zmin && L < zmax && n < kRdMaxLevels) lev[n++] = L;
    }
    if (n == 0) lev[n++] = zmin;
    return n;
}

// Pillow's ImagingBlend (libImaging/Blend.c) of one 8-bit channel: in float, truncated; clipped to 0..255 when alpha is outside [0, 1]
__device__ __forceinline__ uint32_t rd_blend(uint32_t in1, uint32_t in2, float alpha)
{
    const float v = __fadd_rn((float)(int)in1, __fmul_rn(alpha, (float)((int)in2 - (int)in1)));
    if (alpha >= 0.0f && alpha <= 1.0f) return (uint32_t)(uint8_t)(int)v;
    if (v <= 0.0f) return 0u;
    if (v >= 255.0f) return 255u;
    return (uint32_t)(uint8_t)(int)v;
}

// Elevation min / max of each listed table: one workgroup per table
__global__ __launch_bounds__(1024) void k_render_minmax(RenderBgArgs a)
{
    __shared__ double s_lo[1024], s_hi[1024];
    const int t = threadIdx.x;
    const long long n = (long long)a.H * a.W;
    const double *z = a.lay + (long long)a.tabs[blockIdx.x] * a.lay_tab + 4 * n;
    double lo = z[0], hi = z[0];
    for (long long i = t; i < n; i += 1024) { const double v = z[i]; lo = fmin(lo, v); hi = fmax(hi, v); }
    s_lo[t] = lo; s_hi[t] = hi;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (t < w) { s_lo[t] = fmin(s_lo[t], s_lo[t + w]); s_hi[t] = fmax(s_hi[t], s_hi[t + w]); }
        __syncthreads();
    }
    if (t == 0) { a.mm[2 * blockIdx.x] = s_lo[0]; a.mm[2 * blockIdx.x + 1] = s_hi[0]; }
}

// One workgroup: one row of one listed table.  The fuel colour - FuelLayer._update_texture_dryness (layers.py:744-768) for functional
// fuel, FuelModelRGB13 * 255 truncated (layers.py:654-667, sprites.py:136-160) for FBFM codes - and the contour bit: the cell is a
// contour pixel iff min(z, z_n) < L <= max(z, z_n) for a level L and its right or lower neighbour n.
__global__ __launch_bounds__(kRdThreads) void k_render_bg(RenderBgArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_lev[kRdMaxLevels];
    __shared__ int s_n;
    const int y = blockIdx.x, b = blockIdx.y, tab = a.tabs[b];
    if (threadIdx.x == 0) s_n = rd_levels(a.mm[2 * b], a.mm[2 * b + 1], s_lev);
    __syncthreads();
    const int nl = s_n;
    const long long n = (long long)a.H * a.W;
    const double *lay = a.lay + (long long)tab * a.lay_tab;
    const double *z = lay + 4 * n + (long long)y * a.W;
    const bool fbfm = a.fbfm[b] != 0;
    for (int x = threadIdx.x; x < a.W; x += kRdThreads) {
        const long long c = (long long)y * a.W + x;
        uint32_t rgb;
        if (fbfm) {
            const uint32_t ix = a.fuel_ix[(long long)tab * n + c];
            rgb = ix < (uint32_t)kRdFbfmColours ? a.fbfm_rgb[ix] : 0xFFFFFFu;
        } else {
            double pct = lay[c] / 0.2296 + lay[n + c] / 7.0 + (0.2 - lay[2 * n + c]) / 0.2;
            pct = pct / 3.0;
            const float alpha = (float)(pct / 2.0);
            rgb = 0;
            const uint32_t brown[3] = {205u, 133u, 63u};        // DRY_TERRAIN_BROWN_IMG (enums.py:45-47)
            for (int ch = 0; ch < 3; ++ch) rgb |= rd_blend((a.base >> (8 * ch)) & 0xFFu, brown[ch], alpha) << (8 * ch);
        }
        const double v = z[x];
        bool line = false;
        for (int k = 0; k < nl && !line; ++k) {
            const double L = s_lev[k];
            if (x + 1 < a.W) { const double u = z[x + 1]; line |= fmin(v, u) < L && L <= fmax(v, u); }
            if (y + 1 < a.H) { const double u = z[x + a.W]; line |= fmin(v, u) < L && L <= fmax(v, u); }
        }
        a.bg[(long long)tab * n + c] = rgb | (line ? 1u << 24 : 0u);
    }
}

// FBFM code raster -> index into the colour table (kept per table: the codes themselves are dropped after the fuel lookup)
__global__ void k_render_fuel_ix(long long n, const int32_t *codes, const int32_t *table_codes, int n_codes, uint8_t *ix)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t c = codes[i];
    uint8_t r = 255;
    for (int k = 0; k < n_codes; ++k)
        if (table_codes[k] == c) r = (uint8_t)k;
    ix[i] = r;
}

struct RenderArgs {
    Geo g;
    CellPlanes pl;              // the status bytes, in whichever plane is current (read when hist is null)
    const int8_t *hist;         // the history ring [E][cap][H][W] (history source), else null
    int cap, first, count;      // history: frame t of an item shows update first + t (slot (first + t) % cap)
    const uint32_t *bg;         // background words [tables][H * W]
    long long bg_tab;           // words between two tables (0: one shared table)
    const int32_t *envs;        // [n]
    const int32_t *agents;      // [n][k][3] (column, row, id), or null
    uint8_t *out;
    int n_frames, k;            // frames = n * count; agents per item
    int s, mode, white, contours, cl;   // scale, SF_RENDER_NEAREST / MEAN / SPRITES, background white, contours on, channels last
    int oh, ow, R, stride;      // output size, output rows per workgroup, LDS bytes per staged source row (P)
    int st_bytes;               // LDS bytes of the staged region (R * s * stride, rounded to 16)
    int out_seg;                // LDS bytes per output segment (channels last: one of R * ow * 3 + 16; else three of R * ow + 16)
};

// The sprite colours (sprites.py:20-203, enums.py:49, 88-103) and the screen pixel of one cell.  s: status & 7 | kRdAgent.
__device__ __forceinline__ uint32_t rd_cell_rgb(uint32_t s, uint32_t bgw, int white, int contours)
{
    if (s & kRdAgent) return 221u | 160u << 8 | 221u << 16;           // AgentSprite
    switch (s) {
    case 1: return 255u | 153u << 8 | 51u << 16;                      // Fire (BURNING)
    case 3: case 4: return 255u;                                      // FireLine / ScratchLine
    case 5: return 212u | 241u << 8 | 249u << 16;                     // WetLine
    case 2: return 139u | 69u << 8 | 19u << 16;                       // BURNED_RGB_COLOR painted into the terrain image
    default:
        if (contours && (bgw >> 24)) return 0u;                       // contour lines, black
        return white ? 0xFFFFFFu : (bgw & 0xFFFFFFu);
    }
}
// Priority of a cell's sprite for the "sprites" downscale: AGENT > WETLINE > SCRATCHLINE > FIRELINE > BURNING > none
__device__ __forceinline__ int rd_prio(uint32_t s)
{
    if (s & kRdAgent) return 5;
    return s == 5 ? 4 : (s == 4 ? 3 : (s == 3 ? 2 : (s == 1 ? 1 : 0)));
}

// Copy len bytes from LDS (lds + pad lines up with dst modulo 16) to global memory: 16-byte stores, single bytes at both ends
__device__ __forceinline__ void rd_flush(const uint8_t *lds, int pad, uint8_t *dst, int len)
{
    const int t = threadIdx.x;
    const int head = min(len, (16 - pad) & 15);
    const int chunks = (len - head) >> 4;
    for (int i = t; i < head; i += kRdThreads) dst[i] = lds[pad + i];
    for (int c = t; c < chunks; c += kRdThreads)
        *reinterpret_cast<uint4 *>(dst + head + c * 16) = *reinterpret_cast<const uint4 *>(lds + pad + head + c * 16);
    for (int i = head + chunks * 16 + t; i < len; i += kRdThreads) dst[i] = lds[pad + i];
}

// One workgroup: one frame, a band of R output rows.  The band's source rows are staged into LDS once (16-byte loads from either
// plane; the history ring's rows byte by byte unless W is a multiple of 16), the winning agents are flagged in the staged bytes, every
// thread makes output pixels into an LDS copy of the band's output bytes, and the band leaves as whole rows with 16-byte stores.
// Consecutive workgroups are the frames of one band, so a shared background's rows come out of L2.
__global__ __launch_bounds__(kRdThreads) void k_render(RenderArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t rd_lds[];
    uint8_t *st = rd_lds, *ob = rd_lds + a.st_bytes;
    const Geo &g = a.g;
    const int t = threadIdx.x;
    const int fr = (int)(blockIdx.x % (unsigned)a.n_frames), band = (int)(blockIdx.x / (unsigned)a.n_frames);
    const int item = fr / a.count, tt = fr - item * a.count;
    const int e = a.envs[item];
    const int oy0 = band * a.R, orows = min(a.R, a.oh - oy0);
    const int y0 = oy0 * a.s, y1 = min(g.H, (oy0 + orows) * a.s), rows = y1 - y0;

    // stage the band's status bytes (& 7)
    if (a.hist) {
        const int8_t *src = a.hist + ((long long)e * a.cap + (a.first + tt) % a.cap) * g.H * g.W;
        if ((g.W & 15) == 0) {
            const int nv = g.W >> 4;
            for (int idx = t; idx < rows * nv; idx += kRdThreads) {
                const int r = idx / nv, j = idx - r * nv;
                const uint4 q = *reinterpret_cast<const uint4 *>(src + (long long)(y0 + r) * g.W + j * 16);
                *reinterpret_cast<uint4 *>(st + r * a.stride + j * 16) = and4(q, 0x07070707u);
            }
        } else {
            for (int idx = t; idx < rows * g.W; idx += kRdThreads) {
                const int r = idx / g.W, x = idx - r * g.W;
                st[r * a.stride + x] = (uint8_t)src[(long long)(y0 + r) * g.W + x] & 7u;
            }
        }
    } else {
        for (int idx = t; idx < rows * g.PV; idx += kRdThreads) {
            const int r = idx / g.PV, v = idx - r * g.PV, y = y0 + r;
            *reinterpret_cast<uint4 *>(st + r * a.stride + v * 16) = and4(*reinterpret_cast<const uint4 *>(cell_status_vec(a.pl, g, e, y, v)), 0x07070707u);
        }
    }
    __syncthreads();
    // agents as update_agent_positions places them on a fresh map (simulation.py:480-499): entry j shows at its cell iff no later
    // entry moves the same id and no later entry writes the same cell; padding (id <= 0, off the grid) takes no part
    if (a.agents && t < a.k) {
        const int32_t *p = a.agents + ((long long)item * a.k + t) * 3;
        const int x = p[0], y = p[1], id = p[2];
        bool win = id > 0 && x >= 0 && x < g.W && y >= 0 && y < g.H;
        for (int m = t + 1; win && m < a.k; ++m) {
            const int32_t *q = a.agents + ((long long)item * a.k + m) * 3;
            const bool real = q[2] > 0 && q[0] >= 0 && q[0] < g.W && q[1] >= 0 && q[1] < g.H;
            if (real && (q[2] == id || (q[0] == x && q[1] == y))) win = false;
        }
        if (win && y >= y0 && y < y1) st[(y - y0) * a.stride + x] |= kRdAgent;
    }
    __syncthreads();

    const uint32_t *bg = a.bg + (long long)e * a.bg_tab;
    const long long oplane = (long long)a.oh * a.ow;
    int pad[3];
    long long gofs[3];
    if (a.cl) {
        gofs[0] = ((long long)fr * oplane + (long long)oy0 * a.ow) * 3;
    } else {
        for (int c = 0; c < 3; ++c) gofs[c] = ((long long)fr * 3 + c) * oplane + (long long)oy0 * a.ow;
    }
    for (int c = 0; c < (a.cl ? 1 : 3); ++c) pad[c] = (int)(((uintptr_t)a.out + gofs[c]) & 15);
    const int s = a.s;
    for (int p = t; p < orows * a.ow; p += kRdThreads) {
        const int r = p / a.ow, ox = p - r * a.ow;
        const int ys = r * s, xs = ox * s;                                        // block origin in staged rows / columns
        const int ye = min(ys + s, rows), xe = min(xs + s, g.W);
        uint32_t rgb;
        if (s == 1 || a.mode == SF_RENDER_NEAREST) {
            rgb = rd_cell_rgb(st[ys * a.stride + xs], bg[(long long)(y0 + ys) * g.W + xs], a.white, a.contours);
        } else {
            int best = 0;
            uint32_t bs = 0, sr = 0, sg = 0, sb = 0;
            for (int y = ys; y < ye; ++y) {
                const uint8_t *row = st + y * a.stride;
                const uint32_t *brow = bg + (long long)(y0 + y) * g.W;
                for (int x = xs; x < xe; ++x) {
                    const uint32_t sv = row[x];
                    const uint32_t c = rd_cell_rgb(sv, brow[x], a.white, a.contours);
                    sr += c & 0xFFu; sg += (c >> 8) & 0xFFu; sb += c >> 16;
                    if (a.mode == SF_RENDER_SPRITES) {
                        const int pr = rd_prio(sv);
                        if (pr > best) { best = pr; bs = c; }
                    }
                }
            }
            if (best > 0) {
                rgb = bs;
            } else {
                const uint32_t n = (uint32_t)((ye - ys) * (xe - xs));
                rgb = (sr + n / 2) / n | ((sg + n / 2) / n) << 8 | ((sb + n / 2) / n) << 16;
            }
        }
        const int o = r * a.ow + ox;
        if (a.cl) {
            uint8_t *d = ob + pad[0] + o * 3;
            d[0] = (uint8_t)rgb; d[1] = (uint8_t)(rgb >> 8); d[2] = (uint8_t)(rgb >> 16);
        } else {
            for (int c = 0; c < 3; ++c) ob[c * a.out_seg + pad[c] + o] = (uint8_t)(rgb >> (8 * c));
        }
    }
    __syncthreads();
    if (a.cl) {
        rd_flush(ob, pad[0], a.out + gofs[0], orows * a.ow * 3);
    } else {
        for (int c = 0; c < 3; ++c) rd_flush(ob + c * a.out_seg, pad[c], a.out + gofs[c], orows * a.ow);
    }
}

}  // namespace
