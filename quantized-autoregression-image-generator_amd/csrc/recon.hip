// Reconstruction evaluation: per-image error sums (pair_error_*) and mean structural similarity (ssim_*) of
// two batches of fp32 images, in fp64.  Each quantity is a sum of per-workgroup partials that depend on one
// image alone, added by one wave per image in one fixed order: no floating-point atomics, equal inputs give
// equal bits, and an image's value does not depend on which other images share its launch.
// Training against SSIM (ssim_tile_maps_kernel, ssim_bwd_kernel): the forward also writes the three partial
// derivatives of every window's score, the backward correlates them with the window once more; fp64 as well.
#include "qarig_common.h"

namespace qarig {

constexpr int PE_CHUNK = 4096;              // elements of one image per workgroup of pair_error_chunk_kernel
constexpr int PE_TRIPS = PE_CHUNK / 1024;   // 256 threads x 4 elements per trip
constexpr int SSIM_TILE = 16;               // outputs per workgroup: 16 x 16, one per thread
constexpr int SSIM_MAX_TAPS = 15;
constexpr int SSIM_MAX_HALO = SSIM_TILE + SSIM_MAX_TAPS - 1;

struct SsimWindow {
    double w[SSIM_MAX_TAPS];
};

__device__ __forceinline__ double recon_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the larger of two magnitudes; a NaN on either side stays
__device__ __forceinline__ double nan_max(double m, double v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ double recon_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nan_max(v, __shfl_xor(v, o, 64));
    return v;
}

// Four consecutive floats: one 16-byte load where the address allows it, four 4-byte loads otherwise.  The
// values, and with them every sum below, are the same either way.
__device__ __forceinline__ float4 load4(const float* p, bool aligned) {
    if (aligned) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

// Workgroup (n, chunk): elements [chunk PE_CHUNK, +PE_CHUNK) of image n.  Thread t owns elements
// 4 (t + 256 j) ... + 3 of the chunk for j = 0 ... PE_TRIPS - 1 and adds them in that order; then the 64-lane
// butterfly, then the four waves in ascending order.  part[(n chunks + chunk) 3 + {0,1,2}].
__global__ __launch_bounds__(256) void pair_error_chunk_kernel(const float* __restrict__ a,
                                                               const float* __restrict__ b, int64_t E,
                                                               int64_t chunks, double* __restrict__ part) {
    __shared__ double red[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n = (int64_t)blockIdx.x / chunks;
    const int64_t chunk = (int64_t)blockIdx.x - n * chunks;
    const int64_t e0 = chunk * PE_CHUNK;
    const float* pa = a + n * E + e0;
    const float* pb = b + n * E + e0;
    const int64_t left = E - e0;                       // >= 1
    const bool va = (reinterpret_cast<uintptr_t>(pa) & 15) == 0;
    const bool vb = (reinterpret_cast<uintptr_t>(pb) & 15) == 0;
    double s2 = 0.0, s1 = 0.0, mx = 0.0;
#pragma unroll
    for (int j = 0; j < PE_TRIPS; ++j) {
        const int o = 4 * (tid + 256 * j);
        float x[4], y[4];
        int cnt = 4;
        if (o + 4 <= left) {
            const float4 p = load4(pa + o, va), q = load4(pb + o, vb);
            x[0] = p.x; x[1] = p.y; x[2] = p.z; x[3] = p.w;
            y[0] = q.x; y[1] = q.y; y[2] = q.z; y[3] = q.w;
        } else {
            cnt = o < left ? (int)(left - o) : 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                x[i] = i < cnt ? pa[o + i] : 0.0f;
                y[i] = i < cnt ? pb[o + i] : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < cnt) {
                const double d = (double)x[i] - (double)y[i];
                const double ad = fabs(d);
                s2 += d * d;
                s1 += ad;
                mx = nan_max(mx, ad);
            }
        }
    }
    s2 = recon_wave_sum(s2);
    s1 = recon_wave_sum(s1);
    mx = recon_wave_max(mx);
    if (lane == 0) {
        red[wave][0] = s2;
        red[wave][1] = s1;
        red[wave][2] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        double t2 = red[0][0], t1 = red[0][1], tm = red[0][2];
        for (int w = 1; w < 4; ++w) {
            t2 += red[w][0];
            t1 += red[w][1];
            tm = nan_max(tm, red[w][2]);
        }
        double* p = part + (int64_t)blockIdx.x * 3;
        p[0] = t2;
        p[1] = t1;
        p[2] = tm;
    }
}

// One wave per image: lane l adds chunk partials l, l + 64, ... in ascending order, then the butterfly.
__global__ __launch_bounds__(256) void pair_error_finish_kernel(const double* __restrict__ part, int N,
                                                                int64_t chunks, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const double* p = part + n * chunks * 3;
    double s2 = 0.0, s1 = 0.0, mx = 0.0;
    for (int64_t c = lane; c < chunks; c += 64) {
        s2 += p[c * 3];
        s1 += p[c * 3 + 1];
        mx = nan_max(mx, p[c * 3 + 2]);
    }
    s2 = recon_wave_sum(s2);
    s1 = recon_wave_sum(s1);
    mx = recon_wave_max(mx);
    if (lane == 0) {
        out[n * 3] = s2;
        out[n * 3 + 1] = s1;
        out[n * 3 + 2] = mx;
    }
}

// Workgroup (n, c, tile): the 16 x 16 outputs at (ty 16, tx 16) of channel c of image n.  Both images' halo
// of (16 + taps - 1)^2 pixels goes to LDS (zero past the image: only outputs outside the valid region read it,
// and those are dropped), a horizontal pass leaves the five window moments of every (halo row, output column)
// in LDS as doubles, a vertical pass gives each thread its output.  part[block] = sum of the tile's map.
//
// MAPS: each valid position also writes the derivatives of its score v = A1 A2 / (B1 B2) with respect to the
// window moments of a, P = dv/dmx, Q = dv/dxx, R = dv/dxy, to maps (3, planes, oh, ow).  v itself, and with it
// part[], is computed by the same instructions either way.
template <bool MAPS>
__device__ __forceinline__ void ssim_tile(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                          int taps, const SsimWindow& win, double c1, double c2, int tiles_x,
                                          int tiles_y, double* __restrict__ part, double* __restrict__ maps,
                                          int64_t planes) {
    __shared__ float sa[SSIM_MAX_HALO * SSIM_MAX_HALO];
    __shared__ float sb[SSIM_MAX_HALO * SSIM_MAX_HALO];
    __shared__ double hm[5][SSIM_MAX_HALO * SSIM_TILE];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles = tiles_x * tiles_y;
    const int64_t plane = (int64_t)blockIdx.x / tiles;            // n C + c
    const int tile = (int)((int64_t)blockIdx.x - plane * tiles);
    const int ty0 = (tile / tiles_x) * SSIM_TILE, tx0 = (tile % tiles_x) * SSIM_TILE;
    const int halo = SSIM_TILE + taps - 1;
    const float* pa = a + plane * H * W;
    const float* pb = b + plane * H * W;
    for (int i = tid; i < halo * halo; i += 256) {
        const int r = i / halo, q = i - r * halo;
        const int y = ty0 + r, x = tx0 + q;
        const bool in = y < H && x < W;
        const int64_t at = (int64_t)y * W + x;
        sa[i] = in ? pa[at] : 0.0f;
        sb[i] = in ? pb[at] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < halo * SSIM_TILE; i += 256) {
        const int r = i >> 4, ox = i & 15;
        const float* ra = sa + r * halo + ox;
        const float* rb = sb + r * halo + ox;
        double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
        for (int k = 0; k < taps; ++k) {
            const double w = win.w[k], x = (double)ra[k], y = (double)rb[k];
            mx = fma(w, x, mx);
            my = fma(w, y, my);
            xx = fma(w, x * x, xx);          // products of two fp32 values: exact in fp64
            yy = fma(w, y * y, yy);
            xy = fma(w, x * y, xy);
        }
        hm[0][i] = mx;
        hm[1][i] = my;
        hm[2][i] = xx;
        hm[3][i] = yy;
        hm[4][i] = xy;
    }
    __syncthreads();
    const int oy = tid >> 4, ox = tid & 15;
    double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
    for (int k = 0; k < taps; ++k) {
        const double w = win.w[k];
        const int at = (oy + k) * SSIM_TILE + ox;
        mx = fma(w, hm[0][at], mx);
        my = fma(w, hm[1][at], my);
        xx = fma(w, hm[2][at], xx);
        yy = fma(w, hm[3][at], yy);
        xy = fma(w, hm[4][at], xy);
    }
    const double vx = xx - mx * mx, vy = yy - my * my, cov = xy - mx * my;
    const double v = ((2.0 * mx * my + c1) * (2.0 * cov + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2));
    const bool valid = ty0 + oy < H - taps + 1 && tx0 + ox < W - taps + 1;
    if (MAPS && valid) {
        const int oh = H - taps + 1, ow = W - taps + 1;
        const double a1 = 2.0 * mx * my + c1, a2 = 2.0 * cov + c2;
        const double b1 = mx * mx + my * my + c1, b2 = vx + vy + c2;
        const double rb = 1.0 / (b1 * b2);
        const int64_t map = (int64_t)oh * ow;
        double* m = maps + plane * map + (int64_t)(ty0 + oy) * ow + (tx0 + ox);
        m[0] = 2.0 * my * (a2 - a1) * rb - 2.0 * mx * v * (1.0 / b1 - 1.0 / b2);
        m[planes * map] = -v / b2;
        m[2 * planes * map] = 2.0 * a1 * rb;
    }
    double s = recon_wave_sum(valid ? v : 0.0);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (tid == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        int C, int H, int W, int taps, SsimWindow win, double c1,
                                                        double c2, int tiles_x, int tiles_y,
                                                        double* __restrict__ part) {
    ssim_tile<false>(a, b, H, W, taps, win, c1, c2, tiles_x, tiles_y, part, nullptr, 0);
}

__global__ __launch_bounds__(256) void ssim_tile_maps_kernel(const float* __restrict__ a,
                                                             const float* __restrict__ b, int H, int W, int taps,
                                                             SsimWindow win, double c1, double c2, int tiles_x,
                                                             int tiles_y, double* __restrict__ part,
                                                             double* __restrict__ maps, int64_t planes) {
    ssim_tile<true>(a, b, H, W, taps, win, c1, c2, tiles_x, tiles_y, part, maps, planes);
}

// Workgroup (plane, tile): the 16 x 16 INPUT pixels at (ty 16, tx 16) of plane n C + c.  A pixel q belongs to the
// windows of the positions q - (i,j), 0 <= i, j < taps, with weight w_i w_j, so
//   da(q) = g[n] / count * sum_ij w_i w_j [P + 2 a(q) Q + b(q) R](q - (i,j))
// over the valid positions: three correlations of the maps with the window, combined with the thread's own
// pixels.  The halo of (16 + taps - 1)^2 entries of each map starts taps - 1 before the tile and is zero past
// the valid region; a horizontal pass into LDS, a vertical pass with one pixel per thread, all fp64 fma.  Every
// pixel of da is written by exactly one thread.
__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       const double* __restrict__ maps,
                                                       const double* __restrict__ g, int C, int H, int W, int taps,
                                                       SsimWindow win, double count, int tiles_x, int tiles_y,
                                                       int64_t planes, float* __restrict__ da) {
    __shared__ double sm[3][SSIM_MAX_HALO * SSIM_MAX_HALO];
    __shared__ double hm[3][SSIM_MAX_HALO * SSIM_TILE];
    const int tid = threadIdx.x;
    const int tiles = tiles_x * tiles_y;
    const int64_t plane = (int64_t)blockIdx.x / tiles;            // n C + c
    const int tile = (int)((int64_t)blockIdx.x - plane * tiles);
    const int ty0 = (tile / tiles_x) * SSIM_TILE, tx0 = (tile % tiles_x) * SSIM_TILE;
    const int halo = SSIM_TILE + taps - 1;
    const int oh = H - taps + 1, ow = W - taps + 1;
    const int64_t map = (int64_t)oh * ow;
    const double* pm = maps + plane * map;
    for (int i = tid; i < halo * halo; i += 256) {
        const int r = i / halo, q = i - r * halo;
        const int y = ty0 - (taps - 1) + r, x = tx0 - (taps - 1) + q;
        const bool in = y >= 0 && y < oh && x >= 0 && x < ow;
        const int64_t at = (int64_t)y * ow + x;
        sm[0][i] = in ? pm[at] : 0.0;
        sm[1][i] = in ? pm[planes * map + at] : 0.0;
        sm[2][i] = in ? pm[2 * planes * map + at] : 0.0;
    }
    __syncthreads();
    for (int i = tid; i < halo * SSIM_TILE; i += 256) {
        const int r = i >> 4, ox = i & 15;
        const int at = r * halo + ox + taps - 1;                  // position q.x - j is halo column ox + taps - 1 - j
        double p = 0.0, q = 0.0, rr = 0.0;
        for (int k = 0; k < taps; ++k) {
            const double w = win.w[k];
            p = fma(w, sm[0][at - k], p);
            q = fma(w, sm[1][at - k], q);
            rr = fma(w, sm[2][at - k], rr);
        }
        hm[0][i] = p;
        hm[1][i] = q;
        hm[2][i] = rr;
    }
    __syncthreads();
    const int oy = tid >> 4, ox = tid & 15;
    double p = 0.0, q = 0.0, rr = 0.0;
    for (int k = 0; k < taps; ++k) {
        const double w = win.w[k];
        const int at = (oy + taps - 1 - k) * SSIM_TILE + ox;
        p = fma(w, hm[0][at], p);
        q = fma(w, hm[1][at], q);
        rr = fma(w, hm[2][at], rr);
    }
    const int y = ty0 + oy, x = tx0 + ox;
    if (y < H && x < W) {
        const int64_t at = plane * H * W + (int64_t)y * W + x;
        const double d = fma((double)b[at], rr, fma(2.0 * (double)a[at], q, p));
        da[at] = (float)(d * (g[plane / C] / count));
    }
}

// One wave per image: lane l adds partials l, l + 64, ... of the image's C x tiles in ascending (channel,
// tile) order, then the butterfly; the mean over C (H - taps + 1)(W - taps + 1) positions.
__global__ __launch_bounds__(256) void ssim_finish_kernel(const double* __restrict__ part, int N, int64_t per_image,
                                                          double count, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const double* p = part + n * per_image;
    double s = 0.0;
    for (int64_t i = lane; i < per_image; i += 64) s += p[i];
    s = recon_wave_sum(s);
    if (lane == 0) out[n] = s / count;
}

static inline int64_t pe_chunks(int64_t E) { return (E + PE_CHUNK - 1) / PE_CHUNK; }

}  // namespace qarig

using namespace qarig;

// the extents qarig_pair_error accepts, and nothing else
static inline bool pe_extents_ok(int N, int64_t E) {
    return qarig_dims_ok({N, E}, 1LL << 40) && N <= (1 << 24) && (int64_t)N * pe_chunks(E) < (1LL << 31);
}

extern "C" size_t qarig_pair_error_workspace_bytes(int N, int64_t E) {
    if (!pe_extents_ok(N, E)) return 0;
    return (size_t)N * (size_t)pe_chunks(E) * 3 * sizeof(double);
}

// a, b: N contiguous images of E fp32 elements (base pointers 4-byte aligned); out (N,3) fp64, written:
// {sum (a-b)^2, sum |a-b|, max |a-b|} per image, differences, squares and sums in fp64.
extern "C" int qarig_pair_error(const float* a, const float* b, int N, int64_t E, double* out, void* ws,
                                size_t ws_bytes, void* stream) {
    QARIG_CHECK_ARG(a && b && out && ws, "pair_error: null pointer");
    QARIG_CHECK_ARG(qarig_dims_ok({N, E}, 1LL << 40) && N <= (1 << 24),
                    "pair_error: need 1 <= N <= 2^24, E >= 1, N E <= 2^40");
    const int64_t chunks = pe_chunks(E);
    QARIG_CHECK_ARG(pe_extents_ok(N, E), "pair_error: N ceil(E / 4096) must be below 2^31");
    QARIG_CHECK_ARG(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3) == 0 &&
                        (reinterpret_cast<uintptr_t>(out) & 7) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                    "pair_error: a and b must be 4-byte aligned, out and ws 8-byte aligned");
    const size_t need = (size_t)N * (size_t)chunks * 3 * sizeof(double);
    QARIG_CHECK_ARG(ws_bytes >= need, "pair_error: workspace of %zu bytes, %zu needed", ws_bytes, need);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(pair_error_chunk_kernel, dim3((unsigned)(N * chunks)), dim3(256), 0, (hipStream_t)stream, a, b,
                       E, chunks, part);
    QARIG_CHECK_LAUNCH("pair_error");
    hipLaunchKernelGGL(pair_error_finish_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       part, N, chunks, out);
    QARIG_CHECK_LAUNCH("pair_error (finish)");
    return QARIG_OK;
}

static inline bool ssim_geometry(int N, int C, int H, int W, int taps, int64_t* tiles_x, int64_t* tiles_y) {
    if (!qarig_dims_ok({N, C, H, W}) || taps < 1 || taps > SSIM_MAX_TAPS || !(taps & 1) || H < taps || W < taps)
        return false;
    *tiles_x = ((int64_t)W - taps + 1 + SSIM_TILE - 1) / SSIM_TILE;
    *tiles_y = ((int64_t)H - taps + 1 + SSIM_TILE - 1) / SSIM_TILE;
    return true;
}
// one workgroup per (image, channel, tile): tiles_x <= W and tiles_y <= H, so the product is at most N C H W <= 2^40
static inline bool ssim_grid_ok(int N, int C, int64_t tiles_x, int64_t tiles_y) {
    return (int64_t)N * C * tiles_x * tiles_y < (1LL << 31);
}

extern "C" size_t qarig_ssim_workspace_bytes(int N, int C, int H, int W, int taps) {
    int64_t tx, ty;
    if (!ssim_geometry(N, C, H, W, taps, &tx, &ty) || !ssim_grid_ok(N, C, tx, ty)) return 0;
    return (size_t)N * (size_t)C * (size_t)(tx * ty) * sizeof(double);
}

// a, b (N,C,H,W) fp32 contiguous; win: HOST array of `taps` fp64 weights of the separable window; out (N) fp64,
// written: the mean over channels and the (H - taps + 1)(W - taps + 1) valid positions of
// (2 mx my + c1)(2 sxy + c2) / ((mx^2 + my^2 + c1)(sx^2 + sy^2 + c2)), the window moments in fp64.
extern "C" int qarig_ssim(const float* a, const float* b, int N, int C, int H, int W, const double* win, int taps,
                          double c1, double c2, double* out, void* ws, size_t ws_bytes, void* stream) {
    QARIG_CHECK_ARG(a && b && win && out && ws, "ssim: null pointer");
    QARIG_CHECK_DIMS("ssim", N, C, H, W);
    QARIG_CHECK_ARG(taps >= 1 && taps <= SSIM_MAX_TAPS && (taps & 1), "ssim: taps must be odd, 1 <= taps <= 15, got %d",
                    taps);
    QARIG_CHECK_ARG(H >= taps && W >= taps, "ssim: image of %d x %d is smaller than the window of %d taps", H, W, taps);
    int64_t tx = 0, ty = 0;
    ssim_geometry(N, C, H, W, taps, &tx, &ty);
    QARIG_CHECK_ARG(ssim_grid_ok(N, C, tx, ty), "ssim: N C ceil((H-taps+1)/16) ceil((W-taps+1)/16) must be below 2^31");
    const int64_t per_image = (int64_t)C * tx * ty;
    QARIG_CHECK_ARG(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3) == 0 &&
                        ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(ws) |
                          reinterpret_cast<uintptr_t>(win)) & 7) == 0,
                    "ssim: a and b must be 4-byte aligned, win, out and ws 8-byte aligned");
    const size_t need = (size_t)N * (size_t)per_image * sizeof(double);
    QARIG_CHECK_ARG(ws_bytes >= need, "ssim: workspace of %zu bytes, %zu needed", ws_bytes, need);
    SsimWindow wv;                                          // by value: the kernel sees the caller's doubles
    for (int k = 0; k < SSIM_MAX_TAPS; ++k) wv.w[k] = k < taps ? win[k] : 0.0;
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)(per_image * N)), dim3(256), 0, (hipStream_t)stream, a, b, C, H,
                       W, taps, wv, c1, c2, (int)tx, (int)ty, part);
    QARIG_CHECK_LAUNCH("ssim");
    const double count = (double)C * (double)(H - taps + 1) * (double)(W - taps + 1);
    hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, part, N,
                       per_image, count, out);
    QARIG_CHECK_LAUNCH("ssim (finish)");
    return QARIG_OK;
}

// the backward runs one workgroup per (image, channel, 16 x 16 tile of INPUT pixels): at least as many as the
// forward, so this bound covers both launches of the pair
static inline bool ssim_bwd_grid_ok(int N, int C, int H, int W) {
    return (int64_t)N * C * (((int64_t)H + SSIM_TILE - 1) / SSIM_TILE) * (((int64_t)W + SSIM_TILE - 1) / SSIM_TILE) <
           (1LL << 31);
}

extern "C" size_t qarig_ssim_maps_bytes(int N, int C, int H, int W, int taps) {
    int64_t tx, ty;
    if (!ssim_geometry(N, C, H, W, taps, &tx, &ty) || !ssim_bwd_grid_ok(N, C, H, W)) return 0;
    return (size_t)3 * (size_t)N * (size_t)C * (size_t)(H - taps + 1) * (size_t)(W - taps + 1) * sizeof(double);
}

// the argument checks qarig_ssim_fwd_maps and qarig_ssim_bwd share (those of qarig_ssim, with the backward's grid)
#define SSIM_CHECK_SHAPE(what)                                                                                        \
    QARIG_CHECK_DIMS(what, N, C, H, W);                                                                               \
    QARIG_CHECK_ARG(taps >= 1 && taps <= SSIM_MAX_TAPS && (taps & 1), what ": taps must be odd, 1 <= taps <= 15, got %d", \
                    taps);                                                                                            \
    QARIG_CHECK_ARG(H >= taps && W >= taps, what ": image of %d x %d is smaller than the window of %d taps", H, W, taps); \
    QARIG_CHECK_ARG(ssim_bwd_grid_ok(N, C, H, W), what ": N C ceil(H/16) ceil(W/16) must be below 2^31")

// qarig_ssim that also writes maps (3,N,C,oh,ow) fp64 = {dv/dmx, dv/dxx, dv/dxy} of every valid position's score
// v (the moments of a); out is bit-identical to qarig_ssim's.  ws as for qarig_ssim.
extern "C" int qarig_ssim_fwd_maps(const float* a, const float* b, int N, int C, int H, int W, const double* win,
                                   int taps, double c1, double c2, double* out, double* maps, void* ws,
                                   size_t ws_bytes, void* stream) {
    QARIG_CHECK_ARG(a && b && win && out && maps && ws, "ssim_fwd_maps: null pointer");
    SSIM_CHECK_SHAPE("ssim_fwd_maps");
    int64_t tx = 0, ty = 0;
    ssim_geometry(N, C, H, W, taps, &tx, &ty);
    const int64_t per_image = (int64_t)C * tx * ty;
    QARIG_CHECK_ARG(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3) == 0 &&
                        ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(ws) |
                          reinterpret_cast<uintptr_t>(win) | reinterpret_cast<uintptr_t>(maps)) & 7) == 0,
                    "ssim_fwd_maps: a and b must be 4-byte aligned, win, out, maps and ws 8-byte aligned");
    QARIG_CHECK_ARG((const void*)maps != (const void*)a && (const void*)maps != (const void*)b &&
                        (const void*)maps != (const void*)out && (const void*)maps != ws,
                    "ssim_fwd_maps: maps must not alias a, b, out or ws");
    const size_t need = (size_t)N * (size_t)per_image * sizeof(double);
    QARIG_CHECK_ARG(ws_bytes >= need, "ssim_fwd_maps: workspace of %zu bytes, %zu needed", ws_bytes, need);
    SsimWindow wv;
    for (int k = 0; k < SSIM_MAX_TAPS; ++k) wv.w[k] = k < taps ? win[k] : 0.0;
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(ssim_tile_maps_kernel, dim3((unsigned)(per_image * N)), dim3(256), 0, (hipStream_t)stream, a, b,
                       H, W, taps, wv, c1, c2, (int)tx, (int)ty, part, maps, (int64_t)N * C);
    QARIG_CHECK_LAUNCH("ssim_fwd_maps");
    const double count = (double)C * (double)(H - taps + 1) * (double)(W - taps + 1);
    hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, part, N,
                       per_image, count, out);
    QARIG_CHECK_LAUNCH("ssim_fwd_maps (finish)");
    return QARIG_OK;
}

// da (N,C,H,W) fp32, written in full: the gradient of sum_n g[n] out[n] with respect to a, from the maps of
// qarig_ssim_fwd_maps on the same a, b, win and taps.  g (N) fp64 on the device; win a HOST array as above.
// One launch, no atomics; image n's gradient depends on image n and g[n] alone.
extern "C" int qarig_ssim_bwd(const float* a, const float* b, const double* maps, const double* g, int N, int C, int H,
                              int W, const double* win, int taps, float* da, void* stream) {
    QARIG_CHECK_ARG(a && b && maps && g && win && da, "ssim_bwd: null pointer");
    SSIM_CHECK_SHAPE("ssim_bwd");
    QARIG_CHECK_ARG(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(da)) &
                     3) == 0 &&
                        ((reinterpret_cast<uintptr_t>(maps) | reinterpret_cast<uintptr_t>(g) |
                          reinterpret_cast<uintptr_t>(win)) & 7) == 0,
                    "ssim_bwd: a, b and da must be 4-byte aligned, maps, g and win 8-byte aligned");
    QARIG_CHECK_ARG(da != a && da != b && (const void*)da != (const void*)maps && (const void*)da != (const void*)g,
                    "ssim_bwd: da must not alias a, b, maps or g");
    SsimWindow wv;
    for (int k = 0; k < SSIM_MAX_TAPS; ++k) wv.w[k] = k < taps ? win[k] : 0.0;
    const int tx = (W + SSIM_TILE - 1) / SSIM_TILE, ty = (H + SSIM_TILE - 1) / SSIM_TILE;
    const double count = (double)C * (double)(H - taps + 1) * (double)(W - taps + 1);
    hipLaunchKernelGGL(ssim_bwd_kernel, dim3((unsigned)((int64_t)N * C * tx * ty)), dim3(256), 0, (hipStream_t)stream, a, b,
                       maps, g, C, H, W, taps, wv, count, tx, ty, (int64_t)N * C, da);
    QARIG_CHECK_LAUNCH("ssim_bwd");
    return QARIG_OK;
}
