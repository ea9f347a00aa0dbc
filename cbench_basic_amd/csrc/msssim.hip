// Multi-scale structural similarity (Wang, Simoncelli, Bovik 2003) per image, fused: the distortion metric "ms-ssim".
//
// Reference interface: pytorch_msssim.ms_ssim(x_hat, x, data_range, size_average) as consumed at
//   cbench/benchmark/metrics/pytorch_distortion.py:8,17-18 and cbench/modules/entropy_coder/latent_graph.py:14,92-96.
// The package itself is not available (PARITY-UNPINNED); the algorithm is the one benchmark/ms_ssim.py states in torch ops:
// 11-tap Gaussian window (sigma 1.5, normalised) applied separably without padding, K = (0.01, 0.03), five scales, 2 x 2
// average pooling between them (an odd side zero-padded by one on both ends, divisor 4), relu(cs) of scales 0-3 and
// relu(ssim) of scale 4 raised to the weights and multiplied per (image, channel), mean over channels.
//
// Launches per call: 5 x msssim_scale_kernel + 4 x msssim_pool_kernel + 1 x msssim_finish_kernel.
//   scale : one workgroup per 32 x 32 tile of the map of one (image, channel) plane.  The x / y tile with its 10-sample halo
//           goes to LDS, the horizontal pass leaves the five filtered rows (x, y, xx, yy, xy) in LDS, the vertical pass and
//           the cs / ssim arithmetic stay in registers, and the tile's sum of cs (of ssim at the last scale) is stored as
//           ONE float.  The five filtered maps never reach HBM.
//   pool  : the next level of x and y, one launch for both.
//   finish: one wavefront per image adds the tile sums of every (channel, scale) in an order the image's shape alone fixes
//           (lane-strided, then a butterfly), so a value depends neither on the batch size nor on the image's place in it.
// No float atomics, no allocation and no synchronisation: pyramids and tile sums live in the caller's workspace.
#include "common.h"

using namespace basic;

namespace {

constexpr int kTaps = 11, kHalo = kTaps - 1, kScales = 5;
constexpr int kTile = 32;                       // map tile, kTile x kTile outputs
constexpr int kIn = kTile + kHalo;              // 42: tile + halo
constexpr int kRowsPerThread = 4;
constexpr int kBlock = kTile * kTile / kRowsPerThread;   // 256
constexpr int kWaves = kBlock / kWave;
constexpr int kFinishBlock = kWave;
// LDS: 2 x 42 x 43 + 5 x 42 x 33 floats = 42.2 KiB, three workgroups per compute unit.  Rows are padded by one float: both
// passes read 32 consecutive floats of one row per 32-lane group, which is conflict-free at any row stride; the pad keeps
// the stores of the load phase (42-float rows) off one bank.

struct Window { float g[kTaps]; };
struct Weights { float w[kScales]; };

template <bool LAST>
__global__ __launch_bounds__(kBlock) void msssim_scale_kernel(const float *__restrict__ x, const float *__restrict__ y, int hs, int ws,
                                                              int tiles_x, int ntiles, float c1, float c2, Window win,
                                                              float *__restrict__ partial)
{
    __shared__ float sx[kIn][kIn + 1], sy[kIn][kIn + 1];
    __shared__ float sh[5][kIn][kTile + 1];
    __shared__ float red[kWaves];
    const int tid = threadIdx.x;
    const int plane = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
    const int ty0 = (tile / tiles_x) * kTile, tx0 = (tile % tiles_x) * kTile;
    const int64_t base = static_cast<int64_t>(plane) * hs * ws;
    const float *px = x + base, *py = y + base;

    // samples outside the plane read as 0: they reach only outputs outside the map, which are masked below
    for (int i = tid; i < kIn * kIn; i += kBlock) {
        const int r = i / kIn, c = i % kIn;
        const int gy = ty0 + r, gx = tx0 + c;
        const bool in = gy < hs && gx < ws;
        const int64_t o = static_cast<int64_t>(gy) * ws + gx;
        sx[r][c] = in ? px[o] : 0.f;
        sy[r][c] = in ? py[o] : 0.f;
    }
    __syncthreads();

    for (int i = tid; i < kIn * kTile; i += kBlock) {
        const int r = i / kTile, c = i % kTile;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const float u = sx[r][c + k], v = sy[r][c + k], g = win.g[k];
            a0 = fmaf(g, u, a0);
            a1 = fmaf(g, v, a1);
            a2 = fmaf(g, u * u, a2);
            a3 = fmaf(g, v * v, a3);
            a4 = fmaf(g, u * v, a4);
        }
        sh[0][r][c] = a0; sh[1][r][c] = a1; sh[2][r][c] = a2; sh[3][r][c] = a3; sh[4][r][c] = a4;
    }
    __syncthreads();

    // a thread owns kRowsPerThread consecutive map rows of one column: 14 filtered rows serve its four windows
    const int c = tid % kTile, r0 = (tid / kTile) * kRowsPerThread;
    float acc[kRowsPerThread][5];
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i)
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[i][q] = 0.f;
#pragma unroll
    for (int j = 0; j < kRowsPerThread + kHalo; ++j) {
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = sh[q][r0 + j][c];
#pragma unroll
        for (int i = 0; i < kRowsPerThread; ++i) {
            const int k = j - i;   // tap of row r0 + i; taps arrive in rising order for every row
            if (k >= 0 && k < kTaps) {
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[i][q] = fmaf(win.g[k], v[q], acc[i][q]);
            }
        }
    }

    const int mh = hs - kHalo, mw = ws - kHalo;   // the map
    float sum = 0.f;
    {
        // no contraction here: x == y must give s1 == s2 == s12 and equal numerators and denominators, so exactly 1
#pragma clang fp contract(off)
#pragma unroll
        for (int i = 0; i < kRowsPerThread; ++i) {
            const float mu1 = acc[i][0], mu2 = acc[i][1];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = acc[i][2] - mu1_sq, s2 = acc[i][3] - mu2_sq, s12 = acc[i][4] - mu12;
            float val = (2.f * s12 + c2) / (s1 + s2 + c2);
            if (LAST) val = ((2.f * mu12 + c1) / (mu1_sq + mu2_sq + c1)) * val;
            const bool in = ty0 + r0 + i < mh && tx0 + c < mw;
            sum += in ? val : 0.f;
        }
    }
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) sum += __shfl_xor(sum, m, kWave);
    if (tid % kWave == 0) red[tid / kWave] = sum;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
static_assert(kWaves == 4, "the tile sum adds four wave sums");

// 2 x 2 average pooling of x and y; ph / pw = 1 where that side is odd (zero-padded by one on both ends), divisor always 4
__global__ __launch_bounds__(kBlock) void msssim_pool_kernel(const float *__restrict__ x, const float *__restrict__ y, int hs, int ws,
                                                             int hp, int wp, int ph, int pw, int64_t total,
                                                             float *__restrict__ ox, float *__restrict__ oy)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int j = static_cast<int>(i % wp);
        const int64_t t = i / wp;
        const int r = static_cast<int>(t % hp);
        const int64_t src = (t / hp) * hs * ws;
        const int r0 = 2 * r - ph, c0 = 2 * j - pw;
        const bool ra = r0 >= 0, rb = r0 + 1 < hs, ca = c0 >= 0, cb = c0 + 1 < ws;
        const int64_t o = src + static_cast<int64_t>(r0) * ws + c0;
        const float x00 = ra && ca ? x[o] : 0.f, x01 = ra && cb ? x[o + 1] : 0.f, x10 = rb && ca ? x[o + ws] : 0.f,
                    x11 = rb && cb ? x[o + ws + 1] : 0.f;
        const float y00 = ra && ca ? y[o] : 0.f, y01 = ra && cb ? y[o + 1] : 0.f, y10 = rb && ca ? y[o + ws] : 0.f,
                    y11 = rb && cb ? y[o + ws + 1] : 0.f;
        ox[i] = ((x00 + x01) + (x10 + x11)) * 0.25f;
        oy[i] = ((y00 + y01) + (y10 + y11)) * 0.25f;
    }
}

struct FinishArgs {
    int64_t part_off[kScales];   // floats, from the workspace base: [plane][tile] of each scale
    int ntiles[kScales];
    float count[kScales];        // map elements
};

__global__ __launch_bounds__(kFinishBlock) void msssim_finish_kernel(const float *__restrict__ wsp, FinishArgs a, Weights wt, int channels,
                                                                     float *__restrict__ out, float *__restrict__ terms)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    float img = 0.f;
    for (int c = 0; c < channels; ++c) {
        const int64_t plane = static_cast<int64_t>(b) * channels + c;
        float prod = 1.f;
        for (int s = 0; s < kScales; ++s) {
            const float *p = wsp + a.part_off[s] + plane * a.ntiles[s];
            float sum = 0.f;
            for (int t = lane; t < a.ntiles[s]; t += kWave) sum += p[t];
#pragma unroll
            for (int m = kWave / 2; m > 0; m >>= 1) sum += __shfl_xor(sum, m, kWave);
            const float term = fmaxf(sum / a.count[s], 0.f);   // relu; nothing negative reaches powf
            if (terms && lane == 0) terms[plane * kScales + s] = term;
            prod = term > 0.f ? prod * powf(term, wt.w[s]) : 0.f;
        }
        img += prod;
    }
    if (lane == 0) out[b] = img / static_cast<float>(channels);
}

// Workspace layout, in floats from the base, every section a multiple of 64 floats: levels 1..4 of x, then of y
// ([plane][hs][ws] each), then the tile sums of scales 0..4 ([plane][tile] each).  Pure host arithmetic.
struct Plan {
    int hs[kScales], ws[kScales], tiles_x[kScales], ntiles[kScales];
    int64_t planes, x_off[kScales], y_off[kScales], part_off[kScales], total_floats;
};

inline int64_t round64(int64_t n) { return (n + 63) / 64 * 64; }

bool make_plan(int batch, int channels, int h, int w, Plan *p)
{
    if (batch < 1 || channels < 1 || h <= kHalo * 16 || w <= kHalo * 16) return false;
    const int64_t planes = static_cast<int64_t>(batch) * channels, hw = static_cast<int64_t>(h) * w;
    if (planes > (int64_t(1) << 40) / hw) return false;   // 2^40 pixels: every offset below stays far inside int64
    p->planes = planes;
    int64_t off = 0;
    for (int s = 0; s < kScales; ++s) {
        p->hs[s] = s ? p->hs[s - 1] / 2 + p->hs[s - 1] % 2 : h;
        p->ws[s] = s ? p->ws[s - 1] / 2 + p->ws[s - 1] % 2 : w;
        const int64_t tx = (p->ws[s] - kHalo + kTile - 1) / kTile, ty = (p->hs[s] - kHalo + kTile - 1) / kTile;
        if (planes * tx * ty > INT32_MAX) return false;   // one workgroup per (plane, tile) in a 1-D grid
        p->tiles_x[s] = static_cast<int>(tx);
        p->ntiles[s] = static_cast<int>(tx * ty);
    }
    for (int xy = 0; xy < 2; ++xy)
        for (int s = 1; s < kScales; ++s) {
            (xy ? p->y_off : p->x_off)[s] = off;
            off += round64(planes * p->hs[s] * p->ws[s]);
        }
    p->x_off[0] = p->y_off[0] = -1;   // level 0 is the caller's input
    for (int s = 0; s < kScales; ++s) {
        p->part_off[s] = off;
        off += round64(planes * p->ntiles[s]);
    }
    p->total_floats = off;
    return true;
}

}  // namespace

extern "C" int64_t basic_msssim_workspace_bytes(int batch, int channels, int h, int w)
{
    Plan p;
    if (!make_plan(batch, channels, h, w, &p)) return -1;
    return p.total_floats * static_cast<int64_t>(sizeof(float));
}

extern "C" int basic_msssim_per_image_dev(const float *d_x, const float *d_y, int batch, int channels, int h, int w, float data_range,
                                          void *d_workspace, int64_t workspace_bytes, float *d_msssim, float *d_terms,
                                          void *hip_stream)
{
    BASIC_REQUIRE(batch >= 1 && channels >= 1 && data_range > 0.f, "msssim_per_image: bad argument");
    BASIC_REQUIRE(h > kHalo * 16 && w > kHalo * 16,
                  "msssim_per_image: image side should be larger than 160 for 5 scales of an 11-tap window");
    BASIC_REQUIRE(d_x && d_y && d_workspace && d_msssim, "msssim_per_image: null pointer");
    Plan p;
    BASIC_REQUIRE(make_plan(batch, channels, h, w, &p), "msssim_per_image: batch too large");
    BASIC_REQUIRE(workspace_bytes >= p.total_floats * static_cast<int64_t>(sizeof(float)),
                  "msssim_per_image: workspace smaller than basic_msssim_workspace_bytes");
    BASIC_REQUIRE(reinterpret_cast<uintptr_t>(d_workspace) % sizeof(float) == 0, "msssim_per_image: workspace not float-aligned");

    Window win;
    {
        double g[kTaps], sum = 0;
        for (int i = 0; i < kTaps; ++i) sum += g[i] = exp(-double((i - kTaps / 2) * (i - kTaps / 2)) / (2 * 1.5 * 1.5));
        for (int i = 0; i < kTaps; ++i) win.g[i] = static_cast<float>(g[i] / sum);
    }
    const Weights wt = {{0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f}};
    const float c1 = (0.01f * data_range) * (0.01f * data_range), c2 = (0.03f * data_range) * (0.03f * data_range);
    float *wsp = static_cast<float *>(d_workspace);
    hipStream_t st = as_stream(hip_stream);

    const float *lx = d_x, *ly = d_y;
    FinishArgs fa;
    for (int s = 0; s < kScales; ++s) {
        const dim3 grid(static_cast<unsigned>(p.planes * p.ntiles[s]));
        if (s < kScales - 1)
            hipLaunchKernelGGL(msssim_scale_kernel<false>, grid, dim3(kBlock), 0, st, lx, ly, p.hs[s], p.ws[s], p.tiles_x[s], p.ntiles[s],
                               c1, c2, win, wsp + p.part_off[s]);
        else
            hipLaunchKernelGGL(msssim_scale_kernel<true>, grid, dim3(kBlock), 0, st, lx, ly, p.hs[s], p.ws[s], p.tiles_x[s], p.ntiles[s],
                               c1, c2, win, wsp + p.part_off[s]);
        fa.part_off[s] = p.part_off[s];
        fa.ntiles[s] = p.ntiles[s];
        fa.count[s] = static_cast<float>(static_cast<int64_t>(p.hs[s] - kHalo) * (p.ws[s] - kHalo));
        if (s < kScales - 1) {
            const int64_t total = p.planes * p.hs[s + 1] * p.ws[s + 1];
            int64_t g = (total + kBlock - 1) / kBlock;
            if (g > 256 * 8) g = 256 * 8;   // grid-stride the rest
            float *nx = wsp + p.x_off[s + 1], *ny = wsp + p.y_off[s + 1];
            hipLaunchKernelGGL(msssim_pool_kernel, dim3(static_cast<unsigned>(g)), dim3(kBlock), 0, st, lx, ly, p.hs[s], p.ws[s],
                               p.hs[s + 1], p.ws[s + 1], p.hs[s] % 2, p.ws[s] % 2, total, nx, ny);
            lx = nx;
            ly = ny;
        }
    }
    hipLaunchKernelGGL(msssim_finish_kernel, dim3(batch), dim3(kFinishBlock), 0, st, wsp, fa, wt, channels, d_msssim, d_terms);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}
