// 8-bit images: uint8 <-> float32 on the device (include/basic_hip.h section 8b).
//
// What it replaces: the ingest of cbench/data/datasets/torchvision_datasets.py:80-88 (PIL -> ToTensor: HWC uint8 -> CHW
// float32 / 255, a strided copy and a float pass on the host, then four bytes per sample over the bus) and, on the way back,
// the caller's clamp / scale / round / cast of a reconstruction.  Two memory-bound elementwise kernels per direction:
//   wide  : a lane owns four consecutive samples of every channel it touches.  C = 1 is the flat case (BASIC_IMAGE_CHW of any
//           channel count, whose two sides run in the same order): one dword of four samples against one 16-byte float vector.
//           C = 3, 4 is BASIC_IMAGE_HWC with h * w % 4 == 0: four consecutive pixels = C whole dwords against one 16-byte
//           vector per plane.  Needs the uint8 side 4-byte and the float side 16-byte aligned.
//   scalar: one sample per lane per step, any layout, channel count, size and alignment; also the last total % 4 samples of a
//           flat call.
// uint8 -> float32 reads the quotient u / 255 from a 256-entry table: the compiler evaluates float(u) / 255.0f (IEEE, correctly
// rounded) when it builds the table in constant memory, a workgroup copies it to LDS once.  float32 -> uint8 is fmax / fmin /
// one multiply / v_rndne; nothing is contracted into it.
// The third entry measures such pictures: the exact per-channel sum of squared differences of two uint8 batches (further down).
// The last entries cut float tiles out of one uint8 picture, paste reconstructed tiles back into one and, for overlapped tiles, write
// the picture from all their reconstructions with the seams cross-faded (section 8c); the cut and the paste again for tiles of MANY
// pictures, a table row per tile (section 8d, at the end), there also for tiles that leave their picture at the bottom and right: the cut
// replicates the last row and column into them, the paste clips them (the EDGE instantiations).
#include <utility>

#include "common.h"

using namespace basic;

namespace {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 256 * 8;   // memory-bound: eight workgroups per compute unit, grid-stride the rest
constexpr int64_t kMaxSamples = int64_t(1) << 40;

struct QuotientTable {
    float v[256];
    constexpr QuotientTable() : v()
    {
        for (int i = 0; i < 256; ++i) v[i] = static_cast<float>(i) / 255.0f;
    }
};
__constant__ const QuotientTable kQuotients = QuotientTable();

template <int N> struct alignas(4) Words { uint32_t w[N]; };   // N whole dwords: 4 samples of N interleaved channels

__device__ __forceinline__ void load_table(float *lut)
{
    for (int i = threadIdx.x; i < 256; i += kBlock) lut[i] = kQuotients.v[i];
    __syncthreads();
}

__device__ __forceinline__ uint32_t quantise(float x)
{
#pragma clang fp contract(off)
    const float c = fminf(fmaxf(x, 0.f), 1.f);   // fmaxf(NaN, 0) = 0
    return static_cast<uint32_t>(rintf(c * 255.0f));
}

// A run is four consecutive pixels of C interleaved channels, C whole dwords (little-endian: sample p * C + c of the run is pixel
// p, channel c).  Channel c of a run as four floats, and the other way.  Shared by the batch kernels and the tile kernels.
template <int C>
__device__ __forceinline__ float4 run_to_f32(const Words<C> &in, int c, const float *lut)
{
    float o[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int byte = p * C + c;
        o[p] = lut[(in.w[byte / 4] >> (8 * (byte % 4))) & 0xffu];
    }
    return make_float4(o[0], o[1], o[2], o[3]);
}

template <int C>
__device__ __forceinline__ void run_from_f32(Words<C> &out, int c, const float4 &v)   // ORs into `out`: clear it first
{
    const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int byte = p * C + c;
        out.w[byte / 4] |= quantise(x[p]) << (8 * (byte % 4));
    }
}

// run r = (image b, pixels 4 q .. 4 q + 3), runs = runs_per_image * batch.  uint8 side: dwords [r * C, r * C + C).  float
// side: 16-byte vector q of plane b * C + c.  (C = 1: runs_per_image = all runs, both sides flat.)
template <int C>
__global__ __launch_bounds__(kBlock) void u8_to_f32_wide_kernel(const uint32_t *__restrict__ src, float4 *__restrict__ dst,
                                                                 int64_t runs, int64_t runs_per_image)
{
    __shared__ float lut[256];
    load_table(lut);
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; r < runs; r += static_cast<int64_t>(gridDim.x) * kBlock) {
        const Words<C> in = *reinterpret_cast<const Words<C> *>(src + r * C);
        const int64_t b = C == 1 ? 0 : r / runs_per_image, q = C == 1 ? r : r % runs_per_image;
#pragma unroll
        for (int c = 0; c < C; ++c) dst[(b * C + c) * runs_per_image + q] = run_to_f32<C>(in, c, lut);
    }
}

template <int C>
__global__ __launch_bounds__(kBlock) void f32_to_u8_wide_kernel(const float4 *__restrict__ src, uint32_t *__restrict__ dst,
                                                                 int64_t runs, int64_t runs_per_image)
{
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; r < runs; r += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t b = C == 1 ? 0 : r / runs_per_image, q = C == 1 ? r : r % runs_per_image;
        Words<C> out;
#pragma unroll
        for (int k = 0; k < C; ++k) out.w[k] = 0u;
#pragma unroll
        for (int c = 0; c < C; ++c) run_from_f32<C>(out, c, src[(b * C + c) * runs_per_image + q]);
        *reinterpret_cast<Words<C> *>(dst + r * C) = out;
    }
}

// sample i of the float side, i in [first, total): (b, c, p) = (i / (C * P), i / P % C, i % P); its place on the uint8 side
__device__ __forceinline__ int64_t u8_offset(int64_t i, int hwc, int channels, int64_t pixels)
{
    if (!hwc) return i;
    const int64_t p = i % pixels, t = i / pixels;
    return ((t / channels) * pixels + p) * channels + t % channels;
}

__global__ __launch_bounds__(kBlock) void u8_to_f32_scalar_kernel(const uint8_t *__restrict__ src, float *__restrict__ dst, int hwc,
                                                                   int channels, int64_t pixels, int64_t first, int64_t total)
{
    __shared__ float lut[256];
    load_table(lut);
    for (int64_t i = first + static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * kBlock)
        dst[i] = lut[src[u8_offset(i, hwc, channels, pixels)]];
}

// walks the uint8 side (sample j of it, so that the byte stores of a wavefront are consecutive)
__global__ __launch_bounds__(kBlock) void f32_to_u8_scalar_kernel(const float *__restrict__ src, uint8_t *__restrict__ dst, int hwc,
                                                                   int channels, int64_t pixels, int64_t first, int64_t total)
{
    for (int64_t j = first + static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; j < total; j += static_cast<int64_t>(gridDim.x) * kBlock) {
        int64_t i = j;
        if (hwc) {
            const int64_t c = j % channels, t = j / channels;
            i = ((t / pixels) * channels + c) * pixels + t % pixels;
        }
        dst[j] = static_cast<uint8_t>(quantise(src[i]));
    }
}

dim3 grid_for(int64_t work)
{
    const int64_t g = (work + kBlock - 1) / kBlock;
    return dim3(static_cast<unsigned>(g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g));
}

struct Shape {
    int64_t pixels, total;
    int hwc;        // the uint8 side's order differs from the float side's
    int wide_c;     // channels of the wide kernel (1: flat), or 0: sample by sample
};

// the checks both directions share; `what` names the entry in the message
int plan(const void *d_u8, const void *d_f32, int layout, int batch, int channels, int h, int w, const char *what, Shape *s)
{
    const std::string who(what);
    BASIC_REQUIRE(batch >= 1 && channels >= 1 && h >= 1 && w >= 1, who + ": batch, channels, h and w must be positive");
    BASIC_REQUIRE(d_u8 && d_f32, who + ": null pointer");
    BASIC_REQUIRE(layout == BASIC_IMAGE_CHW || layout == BASIC_IMAGE_HWC, who + ": layout is BASIC_IMAGE_CHW or BASIC_IMAGE_HWC");
    BASIC_REQUIRE(reinterpret_cast<uintptr_t>(d_f32) % sizeof(float) == 0, who + ": the float32 pointer is not float-aligned");
    s->pixels = static_cast<int64_t>(h) * w;
    const int64_t planes = static_cast<int64_t>(batch) * channels;
    BASIC_REQUIRE(planes <= kMaxSamples / s->pixels, who + ": more than 2^40 samples");
    s->total = planes * s->pixels;
    s->hwc = layout == BASIC_IMAGE_HWC && channels > 1;   // one channel: the two layouts coincide
    const bool aligned = reinterpret_cast<uintptr_t>(d_u8) % 4 == 0 && reinterpret_cast<uintptr_t>(d_f32) % 16 == 0;
    s->wide_c = !aligned ? 0 : !s->hwc ? 1 : ((channels == 3 || channels == 4) && s->pixels % 4 == 0) ? channels : 0;
    return BASIC_OK;
}

}  // namespace

extern "C" int basic_image_u8_to_f32_dev(const uint8_t *d_src, int layout, int batch, int channels, int h, int w, float *d_dst,
                                         void *hip_stream)
{
    Shape s;
    int rc = plan(d_src, d_dst, layout, batch, channels, h, w, "image_u8_to_f32", &s);
    if (rc) return rc;
    rc = require_device();
    if (rc) return rc;
    hipStream_t st = as_stream(hip_stream);
    const uint32_t *src4 = reinterpret_cast<const uint32_t *>(d_src);
    float4 *dst4 = reinterpret_cast<float4 *>(d_dst);
    int64_t done = 0;   // samples the wide launch covers
    if (s.wide_c == 1) {
        const int64_t runs = s.total / 4;
        if (runs) hipLaunchKernelGGL(u8_to_f32_wide_kernel<1>, grid_for(runs), dim3(kBlock), 0, st, src4, dst4, runs, runs);
        done = runs * 4;
    } else if (s.wide_c) {
        const int64_t rpi = s.pixels / 4, runs = rpi * batch;
        if (s.wide_c == 3) hipLaunchKernelGGL(u8_to_f32_wide_kernel<3>, grid_for(runs), dim3(kBlock), 0, st, src4, dst4, runs, rpi);
        else hipLaunchKernelGGL(u8_to_f32_wide_kernel<4>, grid_for(runs), dim3(kBlock), 0, st, src4, dst4, runs, rpi);
        done = s.total;
    }
    if (done < s.total)
        hipLaunchKernelGGL(u8_to_f32_scalar_kernel, grid_for(s.total - done), dim3(kBlock), 0, st, d_src, d_dst, s.hwc, channels, s.pixels,
                           done, s.total);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_image_f32_to_u8_dev(const float *d_src, int batch, int channels, int h, int w, int layout, uint8_t *d_dst,
                                         void *hip_stream)
{
    Shape s;
    int rc = plan(d_dst, d_src, layout, batch, channels, h, w, "image_f32_to_u8", &s);
    if (rc) return rc;
    rc = require_device();
    if (rc) return rc;
    hipStream_t st = as_stream(hip_stream);
    const float4 *src4 = reinterpret_cast<const float4 *>(d_src);
    uint32_t *dst4 = reinterpret_cast<uint32_t *>(d_dst);
    int64_t done = 0;
    if (s.wide_c == 1) {
        const int64_t runs = s.total / 4;
        if (runs) hipLaunchKernelGGL(f32_to_u8_wide_kernel<1>, grid_for(runs), dim3(kBlock), 0, st, src4, dst4, runs, runs);
        done = runs * 4;
    } else if (s.wide_c) {
        const int64_t rpi = s.pixels / 4, runs = rpi * batch;
        if (s.wide_c == 3) hipLaunchKernelGGL(f32_to_u8_wide_kernel<3>, grid_for(runs), dim3(kBlock), 0, st, src4, dst4, runs, rpi);
        else hipLaunchKernelGGL(f32_to_u8_wide_kernel<4>, grid_for(runs), dim3(kBlock), 0, st, src4, dst4, runs, rpi);
        done = s.total;
    }
    if (done < s.total)
        hipLaunchKernelGGL(f32_to_u8_scalar_kernel, grid_for(s.total - done), dim3(kBlock), 0, st, d_src, d_dst, s.hwc, channels, s.pixels,
                           done, s.total);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

// ---- exact sum of squared differences of two uint8 batches ----------------------------------------------------------------
// d_sse[b][c] = sum over the pixels of (a - b)^2.  Integers only: a lane sums at most 16 squares (<= 1,040,400) in 32 bits,
// adds them to a 64-bit sum of its own, the sums meet by wave shuffles and one LDS word per wave, and a workgroup issues ONE
// 64-bit atomic add per destination it walked, on counters the call has cleared: the same integers for any grid and order.
//   plane : a workgroup walks one (image, channel) plane of both operands; operand X's sample p lies at base_X + p * step_X
//           (CHW: step 1, HWC: step `channels`).  WIDE (both CHW -- or one channel -- and both pointers 4-byte aligned): the
//           plane's whole dwords, one of four samples per lane and operand, four loads in flight; the up to three samples in
//           front of the first whole dword and behind the last (h * w % 4 != 0: a plane does not start on a dword, and the dword
//           around its edge holds samples of two channels or two images) go sample by sample into the sum they belong to.
//           Not WIDE: every sample that way, any layout and alignment.
//   run   : C = 3, 4, at least one operand HWC, h * w % 4 == 0, both pointers 4-byte aligned: a lane owns four consecutive
//           pixels of an image: C whole dwords of an HWC operand, one dword of each plane of a CHW one; C sums per lane.
//           Operand a is the HWC one (the sum is symmetric: the call swaps them).
namespace {

typedef unsigned long long u64;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxGridY = 65535;

__device__ __forceinline__ uint32_t sq_diff(uint32_t x, uint32_t y)
{
    const int d = static_cast<int>(x) - static_cast<int>(y);
    return static_cast<uint32_t>(d * d);
}

// the four squared differences of two dwords of samples
__device__ __forceinline__ uint32_t sq_diff4(uint32_t x, uint32_t y)
{
    return (sq_diff(x & 0xffu, y & 0xffu) + sq_diff((x >> 8) & 0xffu, (y >> 8) & 0xffu)) +
           (sq_diff((x >> 16) & 0xffu, (y >> 16) & 0xffu) + sq_diff(x >> 24, y >> 24));
}

// the workgroup's sum, in every thread; `red` may be used again at once (the next call waits for this one's readers)
__device__ __forceinline__ u64 block_sum(u64 v, u64 *red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 s = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) s += red[k];
    return s;
}

// gridDim.x workgroups share a plane, blockIdx.y strides the planes; plane = image * channels + channel
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void sse_plane_kernel(const uint8_t *__restrict__ a, int hwc_a, const uint8_t *__restrict__ b, int hwc_b,
                                                            int64_t planes, int channels, int64_t pixels, u64 *__restrict__ sse)
{
    __shared__ u64 red[kWaves];
    const int64_t lane = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x, lanes = static_cast<int64_t>(gridDim.x) * kBlock;
    for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const int64_t hwc_base = (plane / channels) * pixels * channels + plane % channels;
        const int64_t base_a = hwc_a ? hwc_base : plane * pixels, base_b = hwc_b ? hwc_base : plane * pixels;
        const int64_t step_a = hwc_a ? channels : 1, step_b = hwc_b ? channels : 1;
        u64 acc = 0;
        int64_t head = 0, tail = 0;   // samples [head, tail) go as dwords, the others one by one
        if (WIDE) {                   // base_a == base_b == plane * pixels, steps of 1
            head = (4 - base_a % 4) % 4;
            if (head > pixels) head = pixels;
            const int64_t n4 = (pixels - head) / 4;
            tail = head + 4 * n4;
            const uint32_t *a4 = reinterpret_cast<const uint32_t *>(a + base_a + head), *b4 = reinterpret_cast<const uint32_t *>(b + base_b + head);
            int64_t i = lane;
            for (; i + 3 * lanes < n4; i += 4 * lanes) {
                const uint32_t x0 = a4[i], x1 = a4[i + lanes], x2 = a4[i + 2 * lanes], x3 = a4[i + 3 * lanes];
                const uint32_t y0 = b4[i], y1 = b4[i + lanes], y2 = b4[i + 2 * lanes], y3 = b4[i + 3 * lanes];
                acc += (sq_diff4(x0, y0) + sq_diff4(x1, y1)) + (sq_diff4(x2, y2) + sq_diff4(x3, y3));   // 16 squares: below 2^20
            }
            for (; i < n4; i += lanes) acc += sq_diff4(a4[i], b4[i]);
        }
        const int64_t singles = pixels - (tail - head);
        for (int64_t p = lane; p < singles; p += lanes) {
            const int64_t q = p < head ? p : p - head + tail;
            acc += sq_diff(a[base_a + q * step_a], b[base_b + q * step_b]);
        }
        const u64 total = block_sum(acc, red);
        if (threadIdx.x == 0) atomicAdd(sse + plane, total);
    }
}

// run q of image `img` = its pixels 4 q .. 4 q + 3.  a: dwords [(img * rpi + q) * C, + C); b: the same (B_HWC) or dword q of
// plane img * C + c.  gridDim.x workgroups share an image, blockIdx.y strides the images.
template <int C, bool B_HWC>
__global__ __launch_bounds__(kBlock) void sse_run_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, int64_t images,
                                                          int64_t runs_per_image, u64 *__restrict__ sse)
{
    __shared__ u64 red[kWaves];
    for (int64_t img = blockIdx.y; img < images; img += gridDim.y) {
        u64 acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0;
        for (int64_t q = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; q < runs_per_image; q += static_cast<int64_t>(gridDim.x) * kBlock) {
            const int64_t r = img * runs_per_image + q;
            const Words<C> wa = *reinterpret_cast<const Words<C> *>(a + r * C);
            Words<C> wb;
            if (B_HWC) {
                wb = *reinterpret_cast<const Words<C> *>(b + r * C);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) wb.w[c] = b[(img * C + c) * runs_per_image + q];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                uint32_t part = 0;   // four squares
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int byte = p * C + c;   // little-endian: sample `byte` of an HWC run
                    const uint32_t x = (wa.w[byte / 4] >> (8 * (byte % 4))) & 0xffu;
                    const uint32_t y = B_HWC ? (wb.w[byte / 4] >> (8 * (byte % 4))) & 0xffu : (wb.w[c] >> (8 * p)) & 0xffu;
                    part += sq_diff(x, y);
                }
                acc[c] += part;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const u64 total = block_sum(acc[c], red);
            if (threadIdx.x == 0) atomicAdd(sse + img * C + c, total);
        }
    }
}

// gridDim of `groups` planes or images of `work` lane steps each: (workgroups that share a group, groups walked side by side)
dim3 sse_grid(int64_t work, int64_t groups)
{
    const int64_t gy = groups < kMaxGridY ? groups : kMaxGridY;
    const int64_t want = (work + kBlock - 1) / kBlock, most = kMaxGrid / gy;
    const int64_t gx = want > most ? most : want;
    return dim3(static_cast<unsigned>(gx < 1 ? 1 : gx), static_cast<unsigned>(gy));
}

}  // namespace

extern "C" int basic_image_sse_u8_dev(const uint8_t *d_a, int layout_a, const uint8_t *d_b, int layout_b, int batch, int channels,
                                      int h, int w, uint64_t *d_sse, void *hip_stream)
{
    const std::string who("image_sse_u8");
    BASIC_REQUIRE(batch >= 1 && channels >= 1 && h >= 1 && w >= 1, who + ": batch, channels, h and w must be positive");
    BASIC_REQUIRE(d_a && d_b && d_sse, who + ": null pointer");
    BASIC_REQUIRE((layout_a == BASIC_IMAGE_CHW || layout_a == BASIC_IMAGE_HWC) && (layout_b == BASIC_IMAGE_CHW || layout_b == BASIC_IMAGE_HWC),
                  who + ": a layout is BASIC_IMAGE_CHW or BASIC_IMAGE_HWC");
    BASIC_REQUIRE(reinterpret_cast<uintptr_t>(d_sse) % sizeof(uint64_t) == 0, who + ": d_sse is not 8-byte aligned");
    const int64_t pixels = static_cast<int64_t>(h) * w, planes = static_cast<int64_t>(batch) * channels;
    BASIC_REQUIRE(planes <= kMaxSamples / pixels, who + ": more than 2^40 samples");
    int rc = require_device();
    if (rc) return rc;
    hipStream_t st = as_stream(hip_stream);
    int hwc_a = layout_a == BASIC_IMAGE_HWC && channels > 1, hwc_b = layout_b == BASIC_IMAGE_HWC && channels > 1;   // one channel: the layouts coincide
    const bool aligned = reinterpret_cast<uintptr_t>(d_a) % 4 == 0 && reinterpret_cast<uintptr_t>(d_b) % 4 == 0;
    u64 *sse = reinterpret_cast<u64 *>(d_sse);
    BASIC_HIP_TRY(hipMemsetAsync(d_sse, 0, static_cast<size_t>(planes) * sizeof(uint64_t), st));   // the workgroups add to it
    if (aligned && (hwc_a || hwc_b) && (channels == 3 || channels == 4) && pixels % 4 == 0) {
        if (!hwc_a) {   // the HWC operand first
            std::swap(d_a, d_b);
            std::swap(hwc_a, hwc_b);
        }
        const uint32_t *a4 = reinterpret_cast<const uint32_t *>(d_a), *b4 = reinterpret_cast<const uint32_t *>(d_b);
        const int64_t images = batch, rpi = pixels / 4;
        const dim3 grid = sse_grid(rpi, images);
        if (channels == 3 && hwc_b) hipLaunchKernelGGL((sse_run_kernel<3, true>), grid, dim3(kBlock), 0, st, a4, b4, images, rpi, sse);
        else if (channels == 3) hipLaunchKernelGGL((sse_run_kernel<3, false>), grid, dim3(kBlock), 0, st, a4, b4, images, rpi, sse);
        else if (hwc_b) hipLaunchKernelGGL((sse_run_kernel<4, true>), grid, dim3(kBlock), 0, st, a4, b4, images, rpi, sse);
        else hipLaunchKernelGGL((sse_run_kernel<4, false>), grid, dim3(kBlock), 0, st, a4, b4, images, rpi, sse);
    } else if (aligned && !hwc_a && !hwc_b) {   // four dwords per lane and pass
        hipLaunchKernelGGL(sse_plane_kernel<true>, sse_grid((pixels + 15) / 16, planes), dim3(kBlock), 0, st, d_a, 0, d_b, 0, planes, channels,
                           pixels, sse);
    } else {
        hipLaunchKernelGGL(sse_plane_kernel<false>, sse_grid(pixels, planes), dim3(kBlock), 0, st, d_a, hwc_a, d_b, hwc_b, planes, channels,
                           pixels, sse);
    }
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

// ---- tiles of one picture (include/basic_hip.h section 8c) -----------------------------------------------------------------
// A tile group is a regular ny x nx grid of th x tw tiles inside ONE uint8 picture; tile t = i * nx + j has its origin at
// (y0 + i * step_y, x0 + j * step_x).  The float side is a batch of tiles, [ny * nx][C][fh][fw]: fh x fw = th x tw when tiles are
// cut out of the picture, sh x sw >= th x tw when reconstructions are pasted back (their top-left th x tw).  One launch per call:
//   wide  : a lane owns four consecutive samples of one tile row, run r = (tile, [channel,] row, q) with q < tw / 4.  PLANAR
//           (C = 1: BASIC_IMAGE_CHW of any channel count) one dword against one 16-byte vector; C = 3, 4 (BASIC_IMAGE_HWC) the
//           C dwords of four pixels against one vector per plane.  img_w, x0, step_x, tw (and sw) are multiples of 4, so every
//           dword of the picture and every vector of the batch is a whole one.
//   scalar: one sample per lane per step; cut walks the float side, paste the uint8 side (consecutive byte stores).
// The values come from the table, quantise() and the run helpers above: the two families cannot drift apart.
namespace {

struct TileGroup {
    int64_t img_h, img_w;                  // the picture
    int64_t y0, x0, step_y, step_x, nx;    // the grid
    int64_t th, tw;                        // a tile
    int64_t fh, fw;                        // a tile's plane on the float side
    int64_t channels;
};

thread_local int g_tiles_last_path = -1;   // basic_image_tiles_last_path: 0 scalar, 1 wide, -1 before any call

// run r of a wide launch -> first sample: offset on the uint8 side (channel 0 when C > 1) and on the float side (plane stride
// fh * fw when C > 1).  Both in samples; both multiples of 4.
// EDGE (section 8d, tiles that leave their picture at the bottom and right): a run is wholly inside or wholly outside a picture row;
// the uint8 offset of an outside run is clamped -- rows at or beyond img_h to row img_h - 1, runs at or beyond img_w to the row's last
// run -- and the result says where the run lay: kRunRight | kRunBelow, 0 inside.  Without EDGE the result is 0.
constexpr int kRunRight = 1, kRunBelow = 2;

template <int C, bool EDGE = false>
__device__ __forceinline__ int locate_run(const TileGroup &g, int64_t r, int64_t *u8, int64_t *f32)
{
    const int64_t qn = g.tw / 4;
    const int64_t q = r % qn, job = r / qn;
    const int64_t row = job % g.th, t = job / g.th;
    const int64_t c = C == 1 ? t % g.channels : 0, tile = C == 1 ? t / g.channels : t;
    int64_t y = g.y0 + (tile / g.nx) * g.step_y + row, x = g.x0 + (tile % g.nx) * g.step_x + 4 * q;
    int where = 0;
    if (EDGE) {
        if (x >= g.img_w) where |= kRunRight, x = g.img_w - 4;
        if (y >= g.img_h) where |= kRunBelow, y = g.img_h - 1;
    }
    *u8 = C == 1 ? (c * g.img_h + y) * g.img_w + x : (y * g.img_w + x) * C;
    *f32 = ((tile * g.channels + c) * g.fh + row) * g.fw + 4 * q;
    return where;
}

// the last pixel of a run in all four places: byte 3 of a planar dword, pixel 3 of an interleaved Words<C>
template <int C>
__device__ __forceinline__ Words<C> broadcast_last(const Words<C> &in)
{
    Words<C> out;
#pragma unroll
    for (int k = 0; k < C; ++k) out.w[k] = 0u;
#pragma unroll
    for (int byte = 0; byte < 4 * C; ++byte) {
        const int from = 3 * C + byte % C;
        out.w[byte / 4] |= ((in.w[from / 4] >> (8 * (from % 4))) & 0xffu) << (8 * (byte % 4));
    }
    return out;
}

// run r of a group, cut and pasted.  Shared by the kernels of one picture here and those of a table of tiles (section 8d).
template <int C, bool EDGE = false>
__device__ __forceinline__ void cut_run(const uint32_t *__restrict__ img, float4 *__restrict__ dst, const TileGroup &g, int64_t r,
                                        const float *lut)
{
    const int64_t plane4 = g.fh * g.fw / 4;
    int64_t u, f;
    const int where = locate_run<C, EDGE>(g, r, &u, &f);
    Words<C> in = *reinterpret_cast<const Words<C> *>(img + u / 4);
    if (EDGE && (where & kRunRight)) in = broadcast_last<C>(in);   // right of the picture: the row's last pixel
#pragma unroll
    for (int c = 0; c < C; ++c) dst[f / 4 + c * plane4] = run_to_f32<C>(in, c, lut);
}

template <int C, bool EDGE = false>
__device__ __forceinline__ void paste_run(const float4 *__restrict__ src, uint32_t *__restrict__ img, const TileGroup &g, int64_t r)
{
    const int64_t plane4 = g.fh * g.fw / 4;
    int64_t u, f;
    if (locate_run<C, EDGE>(g, r, &u, &f)) return;   // outside the picture: nothing is written
    Words<C> out;
#pragma unroll
    for (int k = 0; k < C; ++k) out.w[k] = 0u;
#pragma unroll
    for (int c = 0; c < C; ++c) run_from_f32<C>(out, c, src[f / 4 + c * plane4]);
    *reinterpret_cast<Words<C> *>(img + u / 4) = out;
}

template <int C>
__global__ __launch_bounds__(kBlock) void tiles_u8_to_f32_wide_kernel(const uint32_t *__restrict__ img, float4 *__restrict__ dst,
                                                                       TileGroup g, int64_t runs)
{
    __shared__ float lut[256];
    load_table(lut);
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; r < runs; r += static_cast<int64_t>(gridDim.x) * kBlock)
        cut_run<C>(img, dst, g, r, lut);
}

template <int C>
__global__ __launch_bounds__(kBlock) void tiles_f32_to_u8_wide_kernel(const float4 *__restrict__ src, uint32_t *__restrict__ img,
                                                                       TileGroup g, int64_t runs)
{
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; r < runs; r += static_cast<int64_t>(gridDim.x) * kBlock)
        paste_run<C>(src, img, g, r);
}

// sample (tile, c, row, col) of a group -> its offsets on the two sides
// EDGE: the sample's place in the picture clamped to its last row and column; true when it lay outside (false without EDGE)
template <bool EDGE = false>
__device__ __forceinline__ bool locate_sample(const TileGroup &g, int hwc, int64_t tile, int64_t c, int64_t row, int64_t col, int64_t *u8,
                                              int64_t *f32)
{
    int64_t y = g.y0 + (tile / g.nx) * g.step_y + row, x = g.x0 + (tile % g.nx) * g.step_x + col;
    bool outside = false;
    if (EDGE) {
        outside = y >= g.img_h || x >= g.img_w;
        if (y >= g.img_h) y = g.img_h - 1;
        if (x >= g.img_w) x = g.img_w - 1;
    }
    *u8 = hwc ? (y * g.img_w + x) * g.channels + c : (c * g.img_h + y) * g.img_w + x;
    *f32 = ((tile * g.channels + c) * g.fh + row) * g.fw + col;
    return outside;
}

// sample i of the float side, [tile][c][row][col] (fh x fw = th x tw here), cut
template <bool EDGE = false>
__device__ __forceinline__ void cut_sample(const uint8_t *__restrict__ img, float *__restrict__ dst, int hwc, const TileGroup &g, int64_t i,
                                           const float *lut)
{
    const int64_t col = i % g.tw, job = i / g.tw;
    const int64_t row = job % g.th, t = job / g.th;
    int64_t u, f;
    locate_sample<EDGE>(g, hwc, t / g.channels, t % g.channels, row, col, &u, &f);
    dst[f] = lut[img[u]];
}

// sample j of the uint8 side of the tiles ([tile][c][row][col], hwc: [tile][row][col][c]), pasted
template <bool EDGE = false>
__device__ __forceinline__ void paste_sample(const float *__restrict__ src, uint8_t *__restrict__ img, int hwc, const TileGroup &g, int64_t j)
{
    int64_t tile, c, row, col;
    if (hwc) {
        c = j % g.channels;
        const int64_t t = j / g.channels;
        col = t % g.tw;
        row = t / g.tw % g.th;
        tile = t / g.tw / g.th;
    } else {
        col = j % g.tw;
        const int64_t job = j / g.tw, t = job / g.th;
        row = job % g.th;
        c = t % g.channels;
        tile = t / g.channels;
    }
    int64_t u, f;
    if (locate_sample<EDGE>(g, hwc, tile, c, row, col, &u, &f)) return;   // outside the picture: nothing is written
    img[u] = static_cast<uint8_t>(quantise(src[f]));
}

// walks the float side
__global__ __launch_bounds__(kBlock) void tiles_u8_to_f32_scalar_kernel(const uint8_t *__restrict__ img, float *__restrict__ dst, int hwc,
                                                                         TileGroup g, int64_t total)
{
    __shared__ float lut[256];
    load_table(lut);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * kBlock)
        cut_sample(img, dst, hwc, g, i, lut);
}

// walks the uint8 side of the tiles, so that a wavefront's byte stores are consecutive
__global__ __launch_bounds__(kBlock) void tiles_f32_to_u8_scalar_kernel(const float *__restrict__ src, uint8_t *__restrict__ img, int hwc,
                                                                         TileGroup g, int64_t total)
{
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; j < total; j += static_cast<int64_t>(gridDim.x) * kBlock)
        paste_sample(src, img, hwc, g, j);
}

struct TilePlan {
    TileGroup g;
    int64_t total;   // samples of the tiles: ny * nx * channels * th * tw
    int hwc;
    int wide_c;      // channels of the wide kernel (1: planar), or 0: sample by sample
};

// the checks both directions share; fh x fw is the float side's plane (th x tw for the cut)
int plan_tiles(const void *d_img, const void *d_f32, int layout, int channels, int img_h, int img_w, int y0, int x0, int step_y, int step_x,
               int ny, int nx, int th, int tw, int fh, int fw, const char *what, TilePlan *p, bool may_overlap = false)
{
    const std::string who(what);
    BASIC_REQUIRE(d_img && d_f32, who + ": null pointer");
    BASIC_REQUIRE(layout == BASIC_IMAGE_CHW || layout == BASIC_IMAGE_HWC, who + ": layout is BASIC_IMAGE_CHW or BASIC_IMAGE_HWC");
    BASIC_REQUIRE(channels >= 1 && img_h >= 1 && img_w >= 1 && ny >= 1 && nx >= 1 && th >= 1 && tw >= 1,
                  who + ": channels, the picture's size, ny, nx, th and tw must be positive");
    BASIC_REQUIRE(step_y >= 1 && step_x >= 1, who + ": step_y and step_x must be positive");
    BASIC_REQUIRE(y0 >= 0 && x0 >= 0, who + ": y0 and x0 must not be negative");
    BASIC_REQUIRE(may_overlap || (step_y >= th && step_x >= tw), who + ": a step smaller than the tile (overlapping tiles)");
    BASIC_REQUIRE(fh >= th && fw >= tw, who + ": the source tiles are smaller than th x tw");
    BASIC_REQUIRE(static_cast<int64_t>(y0) + static_cast<int64_t>(ny - 1) * step_y + th <= img_h &&
                      static_cast<int64_t>(x0) + static_cast<int64_t>(nx - 1) * step_x + tw <= img_w,
                  who + ": the last tile leaves the picture");
    BASIC_REQUIRE(reinterpret_cast<uintptr_t>(d_f32) % sizeof(float) == 0, who + ": the float32 pointer is not float-aligned");
    // samples of the float side (the larger of the two): planes * fh * fw <= 2^40, no product overflows on the way
    const int64_t planes = static_cast<int64_t>(ny) * nx;   // < 2^62
    BASIC_REQUIRE(planes <= kMaxSamples / channels, who + ": more than 2^40 samples");
    const int64_t plane = static_cast<int64_t>(fh) * fw;
    BASIC_REQUIRE(planes * channels <= kMaxSamples / plane, who + ": more than 2^40 samples");
    // offsets into the picture stay far inside 64 bits
    BASIC_REQUIRE(static_cast<int64_t>(img_h) * img_w <= (int64_t(1) << 60) / channels, who + ": the picture is too large");
    TileGroup &g = p->g;
    g.img_h = img_h, g.img_w = img_w;
    g.y0 = y0, g.x0 = x0, g.step_y = step_y, g.step_x = step_x, g.nx = nx;
    g.th = th, g.tw = tw, g.fh = fh, g.fw = fw;
    g.channels = channels;
    p->total = planes * channels * th * tw;
    p->hwc = layout == BASIC_IMAGE_HWC && channels > 1;   // one channel: the two layouts coincide
    const bool aligned = reinterpret_cast<uintptr_t>(d_img) % 4 == 0 && reinterpret_cast<uintptr_t>(d_f32) % 16 == 0 && img_w % 4 == 0 &&
                         x0 % 4 == 0 && step_x % 4 == 0 && tw % 4 == 0 && fw % 4 == 0;
    p->wide_c = !aligned ? 0 : !p->hwc ? 1 : (channels == 3 || channels == 4) ? channels : 0;
    return BASIC_OK;
}

}  // namespace

namespace {

// the cut of both entries: the same kernels and the same wide / scalar rule, whether or not the tiles overlap (they are only read)
int cut_tiles(const uint8_t *d_img, int layout, int channels, int img_h, int img_w, int y0, int x0, int step_y, int step_x, int ny, int nx,
              int th, int tw, float *d_dst, void *hip_stream, const char *what, bool may_overlap)
{
    TilePlan p;
    int rc = plan_tiles(d_img, d_dst, layout, channels, img_h, img_w, y0, x0, step_y, step_x, ny, nx, th, tw, th, tw, what, &p, may_overlap);
    if (rc) return rc;
    rc = require_device();
    if (rc) return rc;
    hipStream_t st = as_stream(hip_stream);
    const uint32_t *img4 = reinterpret_cast<const uint32_t *>(d_img);
    float4 *dst4 = reinterpret_cast<float4 *>(d_dst);
    const int64_t runs = p.wide_c == 1 ? p.total / 4 : p.total / 4 / channels;
    if (p.wide_c == 1) hipLaunchKernelGGL(tiles_u8_to_f32_wide_kernel<1>, grid_for(runs), dim3(kBlock), 0, st, img4, dst4, p.g, runs);
    else if (p.wide_c == 3) hipLaunchKernelGGL(tiles_u8_to_f32_wide_kernel<3>, grid_for(runs), dim3(kBlock), 0, st, img4, dst4, p.g, runs);
    else if (p.wide_c == 4) hipLaunchKernelGGL(tiles_u8_to_f32_wide_kernel<4>, grid_for(runs), dim3(kBlock), 0, st, img4, dst4, p.g, runs);
    else hipLaunchKernelGGL(tiles_u8_to_f32_scalar_kernel, grid_for(p.total), dim3(kBlock), 0, st, d_img, d_dst, p.hwc, p.g, p.total);
    g_tiles_last_path = p.wide_c ? 1 : 0;
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

}  // namespace

extern "C" int basic_image_tiles_u8_to_f32_dev(const uint8_t *d_img, int layout, int channels, int img_h, int img_w, int y0, int x0,
                                               int step_y, int step_x, int ny, int nx, int th, int tw, float *d_dst, void *hip_stream)
{
    return cut_tiles(d_img, layout, channels, img_h, img_w, y0, x0, step_y, step_x, ny, nx, th, tw, d_dst, hip_stream, "image_tiles_u8_to_f32", false);
}

extern "C" int basic_image_tiles_overlap_u8_to_f32_dev(const uint8_t *d_img, int layout, int channels, int img_h, int img_w, int y0, int x0,
                                                       int step_y, int step_x, int ny, int nx, int th, int tw, float *d_dst,
                                                       void *hip_stream)
{
    return cut_tiles(d_img, layout, channels, img_h, img_w, y0, x0, step_y, step_x, ny, nx, th, tw, d_dst, hip_stream,
                     "image_tiles_overlap_u8_to_f32", true);
}

extern "C" int basic_image_tiles_f32_to_u8_dev(const float *d_src, int sh, int sw, int channels, int y0, int x0, int step_y, int step_x,
                                               int ny, int nx, int th, int tw, uint8_t *d_img, int layout, int img_h, int img_w,
                                               void *hip_stream)
{
    TilePlan p;
    BASIC_REQUIRE(sh >= 1 && sw >= 1, "image_tiles_f32_to_u8: sh and sw must be positive");
    int rc = plan_tiles(d_img, d_src, layout, channels, img_h, img_w, y0, x0, step_y, step_x, ny, nx, th, tw, sh, sw, "image_tiles_f32_to_u8", &p);
    if (rc) return rc;
    rc = require_device();
    if (rc) return rc;
    hipStream_t st = as_stream(hip_stream);
    const float4 *src4 = reinterpret_cast<const float4 *>(d_src);
    uint32_t *img4 = reinterpret_cast<uint32_t *>(d_img);
    const int64_t runs = p.wide_c == 1 ? p.total / 4 : p.total / 4 / channels;
    if (p.wide_c == 1) hipLaunchKernelGGL(tiles_f32_to_u8_wide_kernel<1>, grid_for(runs), dim3(kBlock), 0, st, src4, img4, p.g, runs);
    else if (p.wide_c == 3) hipLaunchKernelGGL(tiles_f32_to_u8_wide_kernel<3>, grid_for(runs), dim3(kBlock), 0, st, src4, img4, p.g, runs);
    else if (p.wide_c == 4) hipLaunchKernelGGL(tiles_f32_to_u8_wide_kernel<4>, grid_for(runs), dim3(kBlock), 0, st, src4, img4, p.g, runs);
    else hipLaunchKernelGGL(tiles_f32_to_u8_scalar_kernel, grid_for(p.total), dim3(kBlock), 0, st, d_src, d_img, p.hwc, p.g, p.total);
    g_tiles_last_path = p.wide_c ? 1 : 0;
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

// ---- overlapped tiles: the seams cross-faded (include/basic_hip.h section 8c, "Blend") --------------------------------------
// A gather: every output sample of the rectangle is computed from the one, two or four reconstructions that cover it, read where
// decode() left them through a table of (pointer, sh, sw) per tile of the rows x cols grid.  Nothing is accumulated, so a sample's
// value depends on nothing but the tiles that cover it: not on the chunks, the other table entries or the launch shape.
//   axis  : steps s = t - o, n tiles.  Coordinate p lies in tile i = min(p / s, n - 1) at d = p - i * s; with i > 0 and d < o it
//           lies in the band of tiles i - 1 (at d + s) and i (at d), weight ramp(d) = float((2 d + 1) / (2.0 o)).
//   value : lerp(a, b, w) = a + w * (b - a), three rounded fp32 operations, never contracted; x first (top and bottom), then y.
//   wide  : a lane owns four consecutive output samples of one row -- of one plane (PLANAR), or of 3 / 4 interleaved channels.
//           rx0, sx, ox and rw are multiples of 4, so the four share their tiles and band, and their columns inside a source start
//           on a multiple of 4: a 16-byte load where that source's address allows it, four dword loads otherwise (same values).
//   scalar: one output sample per lane per step, walking the output (consecutive stores).
// A null table entry: the samples that need it are not written.  In the wide path the four samples of a run need the same tiles.
namespace {

struct BlendPlan {
    int64_t sy, sx, oy, ox, rows, cols;   // the grid
    int64_t ry0, rx0, rh, rw;             // the output rectangle, in the picture's coordinates
    int64_t channels;
};

struct BlendAxis {
    int64_t ia;      // the (first) covering tile
    int64_t la, lb;  // the coordinate inside tile ia, and inside tile ia + 1 (band only)
    int64_t d;       // distance from the band's start (band only)
    int band;
};

__device__ __forceinline__ BlendAxis blend_axis(int64_t p, int64_t s, int64_t o, int64_t n)
{
    BlendAxis a;
    int64_t i = p / s;
    if (i > n - 1) i = n - 1;
    const int64_t d = p - i * s;
    a.band = i > 0 && d < o;
    a.ia = a.band ? i - 1 : i;
    a.la = a.band ? d + s : d;
    a.lb = d;
    a.d = d;
    return a;
}

__device__ __forceinline__ float blend_ramp(int64_t d, int64_t o)
{
    return static_cast<float>(static_cast<double>(static_cast<int>(2 * d + 1)) / (2.0 * static_cast<int>(o)));   // one double division, rounded once to fp32
}

__device__ __forceinline__ float blend_lerp(float a, float b, float w)
{
#pragma clang fp contract(off)
    const float diff = b - a;
    const float scaled = w * diff;
    return a + scaled;
}

// N consecutive floats of a source plane: row `row`, columns col .. col + N - 1 of channel c
template <int N>
__device__ __forceinline__ void blend_load(const basic_tile_source &e, int64_t c, int64_t row, int64_t col, float *v)
{
    const float *p = e.src + (c * e.sh + row) * static_cast<int64_t>(e.sw) + col;
    if constexpr (N == 4) {
        if (reinterpret_cast<uintptr_t>(p) % 16 == 0) {
            const float4 q = *reinterpret_cast<const float4 *>(p);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = p[k];
}

// N consecutive samples of row `row` of tile row `ti`, cross-faded in x where ax says so; false: a tile they need is missing
template <int N>
__device__ __forceinline__ bool blend_row(const basic_tile_source *__restrict__ table, const BlendPlan &g, int64_t ti, int64_t row, int64_t c,
                                          const BlendAxis &ax, const float *wx, float *v)
{
    const basic_tile_source ea = table[ti * g.cols + ax.ia];
    if (!ea.src) return false;
    blend_load<N>(ea, c, row, ax.la, v);
    if (!ax.band) return true;
    const basic_tile_source eb = table[ti * g.cols + ax.ia + 1];
    if (!eb.src) return false;
    float b[N];
    blend_load<N>(eb, c, row, ax.lb, b);
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = blend_lerp(v[k], b[k], wx[k]);
    return true;
}

// N consecutive samples of picture row y (channel c) that start at the column ax describes
template <int N>
__device__ __forceinline__ bool blend_samples(const basic_tile_source *__restrict__ table, const BlendPlan &g, int64_t c, const BlendAxis &ay,
                                              const BlendAxis &ax, const float *wx, float *v)
{
    if (!blend_row<N>(table, g, ay.ia, ay.la, c, ax, wx, v)) return false;
    if (!ay.band) return true;
    float bottom[N];
    if (!blend_row<N>(table, g, ay.ia + 1, ay.lb, c, ax, wx, bottom)) return false;
    const float wy = blend_ramp(ay.d, g.oy);
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = blend_lerp(v[k], bottom[k], wy);
    return true;
}

// run r: C == 1 (planar) = (channel, row, q) of the rectangle, its four samples at output elements [4 r, 4 r + 4);
// C = 3, 4 (interleaved) = (row, q), its 4 C samples at output elements [4 C r, 4 C r + 4 C), sample p * C + c = pixel p, channel c
template <int C, bool U8>
__global__ __launch_bounds__(kBlock) void tiles_blend_wide_kernel(const basic_tile_source *__restrict__ table, void *__restrict__ out, BlendPlan g,
                                                                   int64_t runs)
{
    const int64_t qn = g.rw / 4;
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; r < runs; r += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t q = r % qn, job = r / qn;
        const int64_t row = C == 1 ? job % g.rh : job, c0 = C == 1 ? job / g.rh : 0;
        const BlendAxis ay = blend_axis(g.ry0 + row, g.sy, g.oy, g.rows), ax = blend_axis(g.rx0 + 4 * q, g.sx, g.ox, g.cols);
        float wx[4] = {0.f, 0.f, 0.f, 0.f};
        if (ax.band) {
#pragma unroll
            for (int k = 0; k < 4; ++k) wx[k] = blend_ramp(ax.d + k, g.ox);
        }
        float v[C][4];
        bool ok = true;
#pragma unroll
        for (int c = 0; c < C; ++c) ok = ok && blend_samples<4>(table, g, c0 + c, ay, ax, wx, v[c]);
        if (!ok) continue;   // a tile is missing: the run keeps its bytes
        if (U8) {
            Words<C> w;
#pragma unroll
            for (int k = 0; k < C; ++k) w.w[k] = 0u;
#pragma unroll
            for (int c = 0; c < C; ++c) run_from_f32<C>(w, c, make_float4(v[c][0], v[c][1], v[c][2], v[c][3]));
            *reinterpret_cast<Words<C> *>(static_cast<uint32_t *>(out) + r * C) = w;
        } else {
            float o[4 * C];
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int p = 0; p < 4; ++p) o[p * C + c] = v[c][p];
#pragma unroll
            for (int k = 0; k < C; ++k) static_cast<float4 *>(out)[r * C + k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        }
    }
}

// output element j of the rectangle: [c][row][col], hwc: [row][col][c]
template <bool U8>
__global__ __launch_bounds__(kBlock) void tiles_blend_scalar_kernel(const basic_tile_source *__restrict__ table, void *__restrict__ out, int hwc,
                                                                     BlendPlan g, int64_t total)
{
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; j < total; j += static_cast<int64_t>(gridDim.x) * kBlock) {
        int64_t c, row, col;
        if (hwc) {
            c = j % g.channels;
            const int64_t t = j / g.channels;
            col = t % g.rw;
            row = t / g.rw;
        } else {
            col = j % g.rw;
            const int64_t t = j / g.rw;
            row = t % g.rh;
            c = t / g.rh;
        }
        const BlendAxis ay = blend_axis(g.ry0 + row, g.sy, g.oy, g.rows), ax = blend_axis(g.rx0 + col, g.sx, g.ox, g.cols);
        const float wx = ax.band ? blend_ramp(ax.d, g.ox) : 0.f;
        float v;
        if (!blend_samples<1>(table, g, c, ay, ax, &wx, &v)) continue;
        if (U8) static_cast<uint8_t *>(out)[j] = static_cast<uint8_t>(quantise(v));
        else static_cast<float *>(out)[j] = v;
    }
}

template <bool U8>
void launch_blend(int wide_c, const basic_tile_source *table, void *out, int hwc, const BlendPlan &g, int64_t total, hipStream_t st)
{
    const int64_t runs = wide_c == 1 ? total / 4 : wide_c ? total / 4 / wide_c : 0;
    if (wide_c == 1) hipLaunchKernelGGL((tiles_blend_wide_kernel<1, U8>), grid_for(runs), dim3(kBlock), 0, st, table, out, g, runs);
    else if (wide_c == 3) hipLaunchKernelGGL((tiles_blend_wide_kernel<3, U8>), grid_for(runs), dim3(kBlock), 0, st, table, out, g, runs);
    else if (wide_c == 4) hipLaunchKernelGGL((tiles_blend_wide_kernel<4, U8>), grid_for(runs), dim3(kBlock), 0, st, table, out, g, runs);
    else hipLaunchKernelGGL(tiles_blend_scalar_kernel<U8>, grid_for(total), dim3(kBlock), 0, st, table, out, hwc, g, total);
}

}  // namespace

extern "C" int basic_image_tiles_blend_dev(const basic_tile_source *d_table, int img_h, int img_w, int th, int tw, int oy, int ox, int channels,
                                           int ry0, int rx0, int rh, int rw, void *d_out, int out_kind, int layout, void *hip_stream)
{
    const std::string who("image_tiles_blend");
    BASIC_REQUIRE(d_table && d_out, who + ": null pointer");
    BASIC_REQUIRE(layout == BASIC_IMAGE_CHW || layout == BASIC_IMAGE_HWC, who + ": layout is BASIC_IMAGE_CHW or BASIC_IMAGE_HWC");
    BASIC_REQUIRE(out_kind == BASIC_PIXEL_U8 || out_kind == BASIC_PIXEL_F32, who + ": out_kind is BASIC_PIXEL_U8 or BASIC_PIXEL_F32");
    BASIC_REQUIRE(channels >= 1 && img_h >= 1 && img_w >= 1 && th >= 1 && tw >= 1 && rh >= 1 && rw >= 1,
                  who + ": channels, the picture's size, th, tw, rh and rw must be positive");
    BASIC_REQUIRE(oy >= 0 && ox >= 0, who + ": oy and ox must not be negative");
    BASIC_REQUIRE(static_cast<int64_t>(2) * oy <= th && static_cast<int64_t>(2) * ox <= tw, who + ": an overlap of more than half a tile");
    BASIC_REQUIRE(ry0 >= 0 && rx0 >= 0 && static_cast<int64_t>(ry0) + rh <= img_h && static_cast<int64_t>(rx0) + rw <= img_w,
                  who + ": the rectangle leaves the picture");
    BASIC_REQUIRE(out_kind != BASIC_PIXEL_F32 || reinterpret_cast<uintptr_t>(d_out) % sizeof(float) == 0,
                  who + ": the float32 output is not float-aligned");
    const int64_t plane = static_cast<int64_t>(rh) * rw;
    BASIC_REQUIRE(channels <= kMaxSamples / plane, who + ": more than 2^40 samples");
    BlendPlan g;
    g.sy = th - oy, g.sx = tw - ox, g.oy = oy, g.ox = ox;
    g.rows = (img_h - oy + g.sy - 1) / g.sy, g.cols = (img_w - ox + g.sx - 1) / g.sx;   // a picture no larger than the overlap: one tile
    if (g.rows < 1) g.rows = 1;
    if (g.cols < 1) g.cols = 1;
    g.ry0 = ry0, g.rx0 = rx0, g.rh = rh, g.rw = rw;
    g.channels = channels;
    int rc = require_device();
    if (rc) return rc;
    const int64_t total = plane * channels;
    const int hwc = layout == BASIC_IMAGE_HWC && channels > 1;   // one channel: the two layouts coincide
    const bool u8 = out_kind == BASIC_PIXEL_U8;
    const bool aligned = reinterpret_cast<uintptr_t>(d_out) % (u8 ? 4 : 16) == 0 && rw % 4 == 0 && rx0 % 4 == 0 && g.sx % 4 == 0 && ox % 4 == 0;
    const int wide_c = !aligned ? 0 : !hwc ? 1 : (channels == 3 || channels == 4) ? channels : 0;
    hipStream_t st = as_stream(hip_stream);
    if (u8) launch_blend<true>(wide_c, d_table, d_out, hwc, g, total, st);
    else launch_blend<false>(wide_c, d_table, d_out, hwc, g, total, st);
    g_tiles_last_path = wide_c ? 1 : 0;
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

// ---- tiles of many pictures (include/basic_hip.h section 8d) ---------------------------------------------------------------
// The cut and the paste above with a table row per tile in place of the grid arithmetic: tile t of the float batch belongs to the
// picture, origin and layout of row t.  blockIdx.y strides the tiles, the workgroups of one blockIdx.y share a tile; a workgroup
// reads its tile's row ONCE, into LDS, and turns it into a TileGroup of one tile, which the run and sample helpers above then
// walk: the values and the access shapes are theirs.  The layout is per row, so a wide launch of C = 3, 4 takes, tile by tile
// (uniformly in a workgroup), the interleaved runs or the planar ones.
namespace {

struct PoolShape {
    int64_t channels, th, tw, fh, fw;   // a tile, and its plane on the float side
};

__device__ __forceinline__ TileGroup pool_group(const basic_tile_ref *__restrict__ table, int64_t t, basic_tile_ref *slot, const PoolShape &s)
{
    __syncthreads();   // the readers of the previous row
    if (threadIdx.x == 0) *slot = table[t];
    __syncthreads();
    TileGroup g;
    g.img_h = slot->img_h, g.img_w = slot->img_w;
    g.y0 = slot->y0, g.x0 = slot->x0, g.step_y = s.th, g.step_x = s.tw, g.nx = 1;
    g.th = s.th, g.tw = s.tw, g.fh = s.fh, g.fw = s.fw;
    g.channels = s.channels;
    return g;
}

// HC: the channels of the rows whose picture is interleaved (3, 4), or 1: every row is planar
template <int HC, bool EDGE = false>
__global__ __launch_bounds__(kBlock) void pool_u8_to_f32_wide_kernel(const basic_tile_ref *__restrict__ table, float4 *__restrict__ dst,
                                                                      PoolShape s, int64_t n)
{
    __shared__ float lut[256];
    __shared__ basic_tile_ref slot;
    load_table(lut);
    const int64_t lane = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x, lanes = static_cast<int64_t>(gridDim.x) * kBlock;
    const int64_t tile4 = s.channels * s.fh * s.fw / 4;
    for (int64_t t = blockIdx.y; t < n; t += gridDim.y) {
        const TileGroup g = pool_group(table, t, &slot, s);
        const uint32_t *img = static_cast<const uint32_t *>(slot.img);
        if (HC > 1 && slot.layout == BASIC_IMAGE_HWC) {
            for (int64_t r = lane; r < s.th * s.tw / 4; r += lanes) cut_run<HC, EDGE>(img, dst + t * tile4, g, r, lut);
        } else {
            for (int64_t r = lane; r < s.channels * s.th * s.tw / 4; r += lanes) cut_run<1, EDGE>(img, dst + t * tile4, g, r, lut);
        }
    }
}

template <int HC, bool EDGE = false>
__global__ __launch_bounds__(kBlock) void pool_f32_to_u8_wide_kernel(const float4 *__restrict__ src, const basic_tile_ref *__restrict__ table,
                                                                      PoolShape s, int64_t n)
{
    __shared__ basic_tile_ref slot;
    const int64_t lane = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x, lanes = static_cast<int64_t>(gridDim.x) * kBlock;
    const int64_t tile4 = s.channels * s.fh * s.fw / 4;
    for (int64_t t = blockIdx.y; t < n; t += gridDim.y) {
        const TileGroup g = pool_group(table, t, &slot, s);
        uint32_t *img = static_cast<uint32_t *>(slot.img);
        if (HC > 1 && slot.layout == BASIC_IMAGE_HWC) {
            for (int64_t r = lane; r < s.th * s.tw / 4; r += lanes) paste_run<HC, EDGE>(src + t * tile4, img, g, r);
        } else {
            for (int64_t r = lane; r < s.channels * s.th * s.tw / 4; r += lanes) paste_run<1, EDGE>(src + t * tile4, img, g, r);
        }
    }
}

template <bool EDGE = false>
__global__ __launch_bounds__(kBlock) void pool_u8_to_f32_scalar_kernel(const basic_tile_ref *__restrict__ table, float *__restrict__ dst,
                                                                        PoolShape s, int64_t n)
{
    __shared__ float lut[256];
    __shared__ basic_tile_ref slot;
    load_table(lut);
    const int64_t lane = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x, lanes = static_cast<int64_t>(gridDim.x) * kBlock;
    const int64_t tile = s.channels * s.fh * s.fw;
    for (int64_t t = blockIdx.y; t < n; t += gridDim.y) {
        const TileGroup g = pool_group(table, t, &slot, s);
        const int hwc = slot.layout == BASIC_IMAGE_HWC && s.channels > 1;
        for (int64_t i = lane; i < s.channels * s.th * s.tw; i += lanes)
            cut_sample<EDGE>(static_cast<const uint8_t *>(slot.img), dst + t * tile, hwc, g, i, lut);
    }
}

template <bool EDGE = false>
__global__ __launch_bounds__(kBlock) void pool_f32_to_u8_scalar_kernel(const float *__restrict__ src, const basic_tile_ref *__restrict__ table,
                                                                        PoolShape s, int64_t n)
{
    __shared__ basic_tile_ref slot;
    const int64_t lane = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x, lanes = static_cast<int64_t>(gridDim.x) * kBlock;
    const int64_t tile = s.channels * s.fh * s.fw;
    for (int64_t t = blockIdx.y; t < n; t += gridDim.y) {
        const TileGroup g = pool_group(table, t, &slot, s);
        const int hwc = slot.layout == BASIC_IMAGE_HWC && s.channels > 1;
        for (int64_t j = lane; j < s.channels * s.th * s.tw; j += lanes)
            paste_sample<EDGE>(src + t * tile, static_cast<uint8_t *>(slot.img), hwc, g, j);
    }
}

struct PoolPlan {
    PoolShape s;
    int wide_c;   // 0: sample by sample; 1: wide, every row planar; 3, 4: wide, interleaved rows of that many channels among them
    dim3 grid;
};

// every check of the entries, on the HOST table: nothing has been copied or launched when this fails.  fh x fw is the float
// side's plane (th x tw for the gather).  edge: tiles may leave their picture at the bottom and right, their origins may not.
int plan_pool(const basic_tile_ref *table, int n, int channels, int th, int tw, int fh, int fw, const void *d_table_ws, const void *d_f32,
              const char *what, PoolPlan *p, bool edge = false)
{
    const std::string who(what);
    BASIC_REQUIRE(table && d_table_ws && d_f32, who + ": null pointer");
    BASIC_REQUIRE(n >= 1, who + ": n must be positive");
    BASIC_REQUIRE(channels >= 1 && th >= 1 && tw >= 1 && fh >= 1 && fw >= 1, who + ": channels and the tile sizes must be positive");
    BASIC_REQUIRE(fh >= th && fw >= tw, who + ": the source tiles are smaller than th x tw");
    BASIC_REQUIRE(reinterpret_cast<uintptr_t>(d_f32) % sizeof(float) == 0, who + ": the float32 pointer is not float-aligned");
    BASIC_REQUIRE(reinterpret_cast<uintptr_t>(d_table_ws) % alignof(basic_tile_ref) == 0, who + ": the table workspace is not 8-byte aligned");
    const int64_t plane = static_cast<int64_t>(fh) * fw;
    BASIC_REQUIRE(static_cast<int64_t>(n) * channels <= kMaxSamples / plane, who + ": more than 2^40 samples");
    bool aligned = reinterpret_cast<uintptr_t>(d_f32) % 16 == 0 && tw % 4 == 0 && fw % 4 == 0;
    bool any_hwc = false;
    for (int t = 0; t < n; ++t) {
        const basic_tile_ref &e = table[t];
        const std::string row = who + ": row " + std::to_string(t);
        BASIC_REQUIRE(e.img, row + ": null picture");
        BASIC_REQUIRE(e.layout == BASIC_IMAGE_CHW || e.layout == BASIC_IMAGE_HWC, row + ": layout is BASIC_IMAGE_CHW or BASIC_IMAGE_HWC");
        BASIC_REQUIRE(e.img_h >= 1 && e.img_w >= 1, row + ": the picture's size must be positive");
        BASIC_REQUIRE(e.y0 >= 0 && e.x0 >= 0, row + ": y0 and x0 must not be negative");
        if (edge) BASIC_REQUIRE(e.y0 < e.img_h && e.x0 < e.img_w, row + ": the tile's origin leaves the picture");
        else BASIC_REQUIRE(static_cast<int64_t>(e.y0) + th <= e.img_h && static_cast<int64_t>(e.x0) + tw <= e.img_w, row + ": the tile leaves the picture");
        BASIC_REQUIRE(static_cast<int64_t>(e.img_h) * e.img_w <= (int64_t(1) << 60) / channels, row + ": the picture is too large");
        const bool hwc = e.layout == BASIC_IMAGE_HWC && channels > 1;   // one channel: the two layouts coincide
        any_hwc = any_hwc || hwc;
        aligned = aligned && reinterpret_cast<uintptr_t>(e.img) % 4 == 0 && e.img_w % 4 == 0 && e.x0 % 4 == 0 &&
                  (!hwc || channels == 3 || channels == 4);
    }
    p->s.channels = channels, p->s.th = th, p->s.tw = tw, p->s.fh = fh, p->s.fw = fw;
    p->wide_c = !aligned ? 0 : any_hwc ? channels : 1;
    const int64_t tile = static_cast<int64_t>(channels) * th * tw;   // a planar row's lanes: no fewer than an interleaved row's
    p->grid = sse_grid(p->wide_c ? tile / 4 : tile, n);              // (workgroups that share a tile, tiles side by side)
    return BASIC_OK;
}

// the table to the caller's workspace, on the stream; returns when the host table may be written again
int stage_pool_table(const basic_tile_ref *table, int n, basic_tile_ref *d_table_ws, hipStream_t st)
{
    BASIC_HIP_TRY(hipMemcpyAsync(d_table_ws, table, static_cast<size_t>(n) * sizeof(basic_tile_ref), hipMemcpyHostToDevice, st));
    BASIC_HIP_TRY(hipStreamSynchronize(st));   // pageable memory: the copy has read it
    return BASIC_OK;
}

}  // namespace

extern "C" int basic_image_tiles_gather_u8_to_f32_dev(const basic_tile_ref *table, int n, int channels, int th, int tw,
                                                      basic_tile_ref *d_table_ws, float *d_dst, void *hip_stream)
{
    PoolPlan p;
    int rc = plan_pool(table, n, channels, th, tw, th, tw, d_table_ws, d_dst, "image_tiles_gather_u8_to_f32", &p);
    if (rc) return rc;
    rc = require_device();
    if (rc) return rc;
    hipStream_t st = as_stream(hip_stream);
    rc = stage_pool_table(table, n, d_table_ws, st);
    if (rc) return rc;
    float4 *dst4 = reinterpret_cast<float4 *>(d_dst);
    const int64_t n64 = n;
    if (p.wide_c == 1) hipLaunchKernelGGL(pool_u8_to_f32_wide_kernel<1>, p.grid, dim3(kBlock), 0, st, d_table_ws, dst4, p.s, n64);
    else if (p.wide_c == 3) hipLaunchKernelGGL(pool_u8_to_f32_wide_kernel<3>, p.grid, dim3(kBlock), 0, st, d_table_ws, dst4, p.s, n64);
    else if (p.wide_c == 4) hipLaunchKernelGGL(pool_u8_to_f32_wide_kernel<4>, p.grid, dim3(kBlock), 0, st, d_table_ws, dst4, p.s, n64);
    else hipLaunchKernelGGL(pool_u8_to_f32_scalar_kernel<>, p.grid, dim3(kBlock), 0, st, d_table_ws, d_dst, p.s, n64);
    g_tiles_last_path = p.wide_c ? 1 : 0;
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_image_tiles_scatter_f32_to_u8_dev(const float *d_src, int sh, int sw, int channels, int th, int tw,
                                                       const basic_tile_ref *table, int n, basic_tile_ref *d_table_ws, void *hip_stream)
{
    PoolPlan p;
    int rc = plan_pool(table, n, channels, th, tw, sh, sw, d_table_ws, d_src, "image_tiles_scatter_f32_to_u8", &p);
    if (rc) return rc;
    rc = require_device();
    if (rc) return rc;
    hipStream_t st = as_stream(hip_stream);
    rc = stage_pool_table(table, n, d_table_ws, st);
    if (rc) return rc;
    const float4 *src4 = reinterpret_cast<const float4 *>(d_src);
    const int64_t n64 = n;
    if (p.wide_c == 1) hipLaunchKernelGGL(pool_f32_to_u8_wide_kernel<1>, p.grid, dim3(kBlock), 0, st, src4, d_table_ws, p.s, n64);
    else if (p.wide_c == 3) hipLaunchKernelGGL(pool_f32_to_u8_wide_kernel<3>, p.grid, dim3(kBlock), 0, st, src4, d_table_ws, p.s, n64);
    else if (p.wide_c == 4) hipLaunchKernelGGL(pool_f32_to_u8_wide_kernel<4>, p.grid, dim3(kBlock), 0, st, src4, d_table_ws, p.s, n64);
    else hipLaunchKernelGGL(pool_f32_to_u8_scalar_kernel<>, p.grid, dim3(kBlock), 0, st, d_src, d_table_ws, p.s, n64);
    g_tiles_last_path = p.wide_c ? 1 : 0;
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

// Edge-padded tiles: the same two launches over tiles of ph x pw that may leave their picture at the bottom and right.  The gather
// replicates the picture's last row and column into the part outside (the clamped address of every sample), the scatter writes the
// part inside and nothing else.  The EDGE instantiations of the kernels above; a table without an edge tile gives the same bits.
extern "C" int basic_image_tiles_gather_pad_u8_to_f32_dev(const basic_tile_ref *table, int n, int channels, int ph, int pw,
                                                          basic_tile_ref *d_table_ws, float *d_dst, void *hip_stream)
{
    PoolPlan p;
    int rc = plan_pool(table, n, channels, ph, pw, ph, pw, d_table_ws, d_dst, "image_tiles_gather_pad_u8_to_f32", &p, true);
    if (rc) return rc;
    rc = require_device();
    if (rc) return rc;
    hipStream_t st = as_stream(hip_stream);
    rc = stage_pool_table(table, n, d_table_ws, st);
    if (rc) return rc;
    float4 *dst4 = reinterpret_cast<float4 *>(d_dst);
    const int64_t n64 = n;
    if (p.wide_c == 1) hipLaunchKernelGGL((pool_u8_to_f32_wide_kernel<1, true>), p.grid, dim3(kBlock), 0, st, d_table_ws, dst4, p.s, n64);
    else if (p.wide_c == 3) hipLaunchKernelGGL((pool_u8_to_f32_wide_kernel<3, true>), p.grid, dim3(kBlock), 0, st, d_table_ws, dst4, p.s, n64);
    else if (p.wide_c == 4) hipLaunchKernelGGL((pool_u8_to_f32_wide_kernel<4, true>), p.grid, dim3(kBlock), 0, st, d_table_ws, dst4, p.s, n64);
    else hipLaunchKernelGGL(pool_u8_to_f32_scalar_kernel<true>, p.grid, dim3(kBlock), 0, st, d_table_ws, d_dst, p.s, n64);
    g_tiles_last_path = p.wide_c ? 1 : 0;
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_image_tiles_scatter_clip_f32_to_u8_dev(const float *d_src, int sh, int sw, int channels, int ph, int pw,
                                                            const basic_tile_ref *table, int n, basic_tile_ref *d_table_ws, void *hip_stream)
{
    PoolPlan p;
    int rc = plan_pool(table, n, channels, ph, pw, sh, sw, d_table_ws, d_src, "image_tiles_scatter_clip_f32_to_u8", &p, true);
    if (rc) return rc;
    rc = require_device();
    if (rc) return rc;
    hipStream_t st = as_stream(hip_stream);
    rc = stage_pool_table(table, n, d_table_ws, st);
    if (rc) return rc;
    const float4 *src4 = reinterpret_cast<const float4 *>(d_src);
    const int64_t n64 = n;
    if (p.wide_c == 1) hipLaunchKernelGGL((pool_f32_to_u8_wide_kernel<1, true>), p.grid, dim3(kBlock), 0, st, src4, d_table_ws, p.s, n64);
    else if (p.wide_c == 3) hipLaunchKernelGGL((pool_f32_to_u8_wide_kernel<3, true>), p.grid, dim3(kBlock), 0, st, src4, d_table_ws, p.s, n64);
    else if (p.wide_c == 4) hipLaunchKernelGGL((pool_f32_to_u8_wide_kernel<4, true>), p.grid, dim3(kBlock), 0, st, src4, d_table_ws, p.s, n64);
    else hipLaunchKernelGGL(pool_f32_to_u8_scalar_kernel<true>, p.grid, dim3(kBlock), 0, st, d_src, d_table_ws, p.s, n64);
    g_tiles_last_path = p.wide_c ? 1 : 0;
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_image_tiles_last_path(int *path)
{
    BASIC_REQUIRE(path, "image_tiles_last_path: null argument");
    *path = g_tiles_last_path;
    return BASIC_OK;
}
