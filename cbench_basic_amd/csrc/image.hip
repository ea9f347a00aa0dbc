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
        for (int c = 0; c < C; ++c) {
            float o[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int byte = p * C + c;   // little-endian: sample `byte` of the run
                o[p] = lut[(in.w[byte / 4] >> (8 * (byte % 4))) & 0xffu];
            }
            dst[(b * C + c) * runs_per_image + q] = make_float4(o[0], o[1], o[2], o[3]);
        }
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
        for (int c = 0; c < C; ++c) {
            const float4 v = src[(b * C + c) * runs_per_image + q];
            const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int byte = p * C + c;
                out.w[byte / 4] |= quantise(x[p]) << (8 * (byte % 4));
            }
        }
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
