// Entropy-parameter kernels: fused quantise + table-index evaluation, coalesced over HBM.
// These are pure streaming kernels (a few bytes in, 8 bytes out per latent): the only rules
// that matter are full-width coalesced accesses and enough workgroups to cover 256 CUs.
//
// Reference semantics:
//   GaussianConditional.build_indexes / quantize  (CompressAI 1.2.3, quoted at
//       modules/prior_model/prior_coder/pgm_coder.py:814-818; call site compressai_coder.py:377-393)
//   EntropyBottleneck.compress/decompress         (call site compressai_coder.py:230-245)
//   GaussianPGMPriorCoderImpl._select_best_indexes pgm_coder.py:802-821
//   TopoGroupPGMPriorCoder group step              pgm_coder.py:921-941, 962-978
#include "ans_common.h"   // clampi, bypass_split, escape_digits: the coder's own split of a value

using namespace basic;

namespace {

constexpr int kBlock = 256;

inline int grid_for(int64_t n)
{
    int64_t g = (n + kBlock - 1) / kBlock;
    if (g > 256 * 8) g = 256 * 8;  // grid-stride the rest
    if (g < 1) g = 1;
    return static_cast<int>(g);
}

// torch.round / rintf: round half to even (v_rndne_f32).
__device__ __forceinline__ float round_even(float v) { return rintf(v); }

__global__ void gc_quantize_index_kernel(const float *__restrict__ y, const float *__restrict__ scales, int64_t n,
                                         const float *__restrict__ table, int table_len, float bound,
                                         int32_t *__restrict__ symbols, int32_t *__restrict__ indexes,
                                         float *__restrict__ yhat)
{
    extern __shared__ float s_table[];
    __shared__ int s_unsorted;
    if (threadIdx.x == 0) s_unsorted = 0;
    for (int i = threadIdx.x; i < table_len; i += blockDim.x) s_table[i] = table[i];
    __syncthreads();
    for (int i = threadIdx.x; i + 1 < table_len; i += blockDim.x)
        if (!(s_table[i] <= s_table[i + 1])) s_unsorted = 1;
    __syncthreads();
    // build_indexes (compressai GaussianConditional): idx = (len - 1) - #{ j < len - 1 : s <= table[j] }.  On a non-decreasing
    // table (the scale table is: checked above) that count is the number of entries from the first one >= s on, so idx is
    // that entry's position, found in log2(len) probes instead of len - 1 compares per element (the kernel was VALU-bound at
    // ten times its HBM time).  NaN and unsorted tables take the counting loop.
    const bool sorted = s_unsorted == 0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const float s = fmaxf(scales[i], bound);  // LowerBound
        int idx;
        if (sorted && s == s) {
            int lo = 0, hi = table_len - 1;   // first j in [0, len - 1) with table[j] >= s, len - 1 if none
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_table[mid] < s) lo = mid + 1; else hi = mid;
            }
            idx = lo;
        } else {
            idx = table_len - 1;
            for (int j = 0; j < table_len - 1; ++j) idx -= (s <= s_table[j]) ? 1 : 0;
        }
        const float q = round_even(y[i]);
        symbols[i] = static_cast<int32_t>(q);
        indexes[i] = idx;
        if (yhat) yhat[i] = q;
    }
}

// ---- quantiser step (include/basic_hip.h, "Quantiser step"): the division and the multiply of the format, each one correctly
// rounded fp32 operation -- no reciprocal, nothing contracted into a neighbour.  The build states
// -fhip-fp32-correctly-rounded-divide-sqrt itself, so the division does not rest on the compiler's default either.
__device__ __forceinline__ float step_div(float a, float step)
{
#pragma clang fp contract(off)
    return __fdiv_rn(a, step);
}
__device__ __forceinline__ float step_mul(float q, float step)
{
#pragma clang fp contract(off)
    return __fmul_rn(q, step);
}

// gc_quantize_index_kernel with a quantiser step per image: element i of image b = i / per_image is coded as rint(y / step[b])
// under the table entry of max(scale, bound) / step[b].  Same streaming shape as the step-less kernel: flat grid-stride over
// B * per_image, full-width coalesced loads and stores.  The image of an element comes from ONE 64-bit division per
// grid-stride chunk, uniform over the workgroup (its chunk's first element), and a walk over the image boundaries that fall
// inside the chunk (none or one unless per_image < 256).
__global__ void gc_quantize_index_q_kernel(const float *__restrict__ y, const float *__restrict__ scales, int64_t n, int64_t per_image,
                                           const float *__restrict__ steps, int n_steps, const float *__restrict__ table,
                                           int table_len, float bound, int32_t *__restrict__ symbols,
                                           int32_t *__restrict__ indexes, float *__restrict__ yhat)
{
    extern __shared__ float s_table[];
    __shared__ int s_unsorted;
    if (threadIdx.x == 0) s_unsorted = 0;
    for (int i = threadIdx.x; i < table_len; i += blockDim.x) s_table[i] = table[i];
    __syncthreads();
    for (int i = threadIdx.x; i + 1 < table_len; i += blockDim.x)
        if (!(s_table[i] <= s_table[i + 1])) s_unsorted = 1;
    __syncthreads();
    const bool sorted = s_unsorted == 0;
    for (int64_t base = static_cast<int64_t>(blockIdx.x) * blockDim.x; base < n; base += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        if (i >= n) break;
        int64_t b = base / per_image;                         // uniform: once per chunk
        int64_t r = (base - b * per_image) + threadIdx.x;
        while (r >= per_image) { r -= per_image; ++b; }        // i < n = B * per_image keeps b < B
        const float step = steps[n_steps == 1 ? 0 : b];
        const float s = step_div(fmaxf(scales[i], bound), step);  // LowerBound first, then the step
        int idx;
        if (sorted && s == s) {
            int lo = 0, hi = table_len - 1;   // first j in [0, len - 1) with table[j] >= s, len - 1 if none
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_table[mid] < s) lo = mid + 1; else hi = mid;
            }
            idx = lo;
        } else {
            idx = table_len - 1;
            for (int j = 0; j < table_len - 1; ++j) idx -= (s <= s_table[j]) ? 1 : 0;
        }
        const float q = round_even(step_div(y[i], step));
        symbols[i] = static_cast<int32_t>(q);
        indexes[i] = idx;
        if (yhat) yhat[i] = step_mul(q, step);
    }
}

// i32_to_f32_kernel with the step: yhat = float(sym) * step[image], the encoder's q * step (its bits for every sym != 0; a
// symbol 0 gives +0.0 where the encoder's rint may have left -0.0, as i32_to_f32_kernel does against gc_quantize_index_kernel)
__global__ void gc_dequantize_q_kernel(const int32_t *__restrict__ in, int64_t n, int64_t per_image, const float *__restrict__ steps,
                                       int n_steps, float *__restrict__ out)
{
    for (int64_t base = static_cast<int64_t>(blockIdx.x) * blockDim.x; base < n; base += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        if (i >= n) break;
        int64_t b = base / per_image;
        int64_t r = (base - b * per_image) + threadIdx.x;
        while (r >= per_image) { r -= per_image; ++b; }
        out[i] = step_mul(static_cast<float>(in[i]), steps[n_steps == 1 ? 0 : b]);
    }
}

// ---- mean-scale hyperprior (include/basic_hip.h, "Mean-scale"): y is coded as rint(y - mu) under the scale's table entry and
// rebuilt as q + mu.  Each helper is one correctly rounded fp32 operation.  They are plain operators under the pragma, as in
// rate_refine_kernel: the *_rn intrinsics are inline functions compiled under the build's own contraction mode, and a multiply
// and an add of theirs that meet after inlining would fuse -- (q * step) + mu is two roundings in the format, never an FMA.
__device__ __forceinline__ float mean_sub(float y, float mu)
{
#pragma clang fp contract(off)
    return y - mu;
}
__device__ __forceinline__ float mean_add(float q, float mu)
{
#pragma clang fp contract(off)
    return q + mu;
}
__device__ __forceinline__ float step_mul_mean_add(float q, float step, float mu)
{
#pragma clang fp contract(off)
    const float p = q * step;
    return p + mu;
}

// gc_quantize_index_q_kernel with a mean per element; kStep == false is the step-less format and carries no division.  Same
// streaming shape: flat grid-stride over B * per_image, the image of a chunk from one 64-bit division.  The parameters of element
// (b, r) lie at b * param_stride + r of `scales` and `means`, so the two halves of a chunked prior [B][2 M][h][w] are read in
// place (means = scales + per_image, param_stride = 2 per_image) and consecutive lanes still read consecutive addresses.
// y == nullptr: indexes only (the decoder), nothing but the scales is read.
template <bool kStep>
__global__ void gc_quantize_index_ms_kernel(const float *__restrict__ y, const float *__restrict__ scales, const float *__restrict__ means,
                                            int64_t n, int64_t per_image, int64_t param_stride, const float *__restrict__ steps,
                                            int n_steps, const float *__restrict__ table, int table_len, float bound,
                                            int32_t *__restrict__ symbols, int32_t *__restrict__ indexes, float *__restrict__ yhat)
{
    extern __shared__ float s_table[];
    __shared__ int s_unsorted;
    if (threadIdx.x == 0) s_unsorted = 0;
    for (int i = threadIdx.x; i < table_len; i += blockDim.x) s_table[i] = table[i];
    __syncthreads();
    for (int i = threadIdx.x; i + 1 < table_len; i += blockDim.x)
        if (!(s_table[i] <= s_table[i + 1])) s_unsorted = 1;
    __syncthreads();
    const bool sorted = s_unsorted == 0;
    for (int64_t base = static_cast<int64_t>(blockIdx.x) * blockDim.x; base < n; base += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        if (i >= n) break;
        int64_t b = base / per_image;                         // uniform: once per chunk
        int64_t r = (base - b * per_image) + threadIdx.x;
        while (r >= per_image) { r -= per_image; ++b; }        // i < n = B * per_image keeps b < B
        const int64_t p = b * param_stride + r;
        float step = 1.f;
        if constexpr (kStep) step = steps[n_steps == 1 ? 0 : b];
        float s = fmaxf(scales[p], bound);  // LowerBound first, then the step
        if constexpr (kStep) s = step_div(s, step);
        int idx;
        if (sorted && s == s) {
            int lo = 0, hi = table_len - 1;   // first j in [0, len - 1) with table[j] >= s, len - 1 if none
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_table[mid] < s) lo = mid + 1; else hi = mid;
            }
            idx = lo;
        } else {
            idx = table_len - 1;
            for (int j = 0; j < table_len - 1; ++j) idx -= (s <= s_table[j]) ? 1 : 0;
        }
        indexes[i] = idx;
        if (y) {
            const float mu = means[p];
            float res = mean_sub(y[i], mu);
            if constexpr (kStep) res = step_div(res, step);
            const float q = round_even(res);
            symbols[i] = static_cast<int32_t>(q);
            if (yhat) {
                if constexpr (kStep) yhat[i] = step_mul_mean_add(q, step, mu);
                else yhat[i] = mean_add(q, mu);
            }
        }
    }
}

// the decoder's yhat = float(sym) + mu, or (float(sym) * step) + mu: the encoder's bits wherever sym != 0 or mu != 0
template <bool kStep>
__global__ void gc_dequantize_ms_kernel(const int32_t *__restrict__ in, const float *__restrict__ means, int64_t n, int64_t per_image,
                                        int64_t param_stride, const float *__restrict__ steps, int n_steps, float *__restrict__ out)
{
    for (int64_t base = static_cast<int64_t>(blockIdx.x) * blockDim.x; base < n; base += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        if (i >= n) break;
        int64_t b = base / per_image;
        int64_t r = (base - b * per_image) + threadIdx.x;
        while (r >= per_image) { r -= per_image; ++b; }
        const float mu = means[b * param_stride + r], q = static_cast<float>(in[i]);
        if constexpr (kStep) out[i] = step_mul_mean_add(q, steps[n_steps == 1 ? 0 : b], mu);
        else out[i] = mean_add(q, mu);
    }
}

// ---- rate control (include/basic_hip.h, "Rate control"): the exact table cost of every stream at each candidate step.
// One read of y and sigma serves all candidates: an element sits in two registers while the candidate loop -- unrolled over the
// template's kNC accumulators, n_cand <= kNC of them live -- repeats gc_quantize_index_q_kernel's arithmetic for the step and
// looks the symbol's cost up (a 4-byte gather from the [rows][stride] table in HBM / L2: the entries around a row's centre are
// the hot ones, see profiles/rate_control.txt).  A workgroup belongs to one segment: workgroup g = (segment g / bps, part g % bps).
// Integer partial sums per lane, then wave (shuffles), workgroup (LDS), and one 64-bit atomic per (workgroup, segment,
// candidate): nothing here rounds, so the sums depend on neither the grid nor the order of arrival.
struct RateTables {
    const uint32_t *cost;
    const int32_t *sizes, *offsets;
    int rows, stride;
    uint32_t bprec;
};
constexpr int kRateMaxRows = 1024;
constexpr int kRateMaxCand = 32;

__device__ __forceinline__ uint32_t symbol_cost(const RateTables &T, const int2 *rowinfo, int32_t row, int32_t sym)
{
    row = clampi(row, 0, T.rows - 1);
    const int2 ri = rowinfo[row];   // (offset, max_value), as the encoder's enc_prepare reads them
    const int32_t max_value = ri.y;
    int32_t value = static_cast<int32_t>(static_cast<uint32_t>(sym) - static_cast<uint32_t>(ri.x));
    uint32_t raw = 0;
    bypass_split(value, max_value, raw);
    const bool escaped = value == max_value;
    value = clampi(value, 0, max_value);
    uint32_t c = T.cost[static_cast<int64_t>(row) * T.stride + value];
    if (escaped) {   // the escape code: nb digits, the count nibble, one more per maxbv digits (encode_escape)
        const uint32_t nb = static_cast<uint32_t>(escape_digits(raw, T.bprec)), maxbv = (1u << T.bprec) - 1u;
        c += (T.bprec * (nb + 1u + nb / maxbv)) << 16;
    }
    return c;
}

//
// kMean (the mean-scale coder): the element's mean is read beside y and the candidate loop works on y - mu, subtracted once; the
// parameters of segment s, image b = s / segs_per_image, start at b * param_stride + (s % segs_per_image) * per_seg of `scales` and
// `means` (gc_quantize_index_ms_kernel's addressing).  Without it neither argument is read.
template <int kNC, bool kMean>
__global__ __launch_bounds__(kBlock) void gc_rate_curve_kernel(const float *__restrict__ y, const float *__restrict__ scales,
                                                               const float *__restrict__ means, int64_t param_stride, int64_t per_seg,
                                                               int segs_per_image, int bps, const float *__restrict__ cand, int n_cand,
                                                               int cand_per_image, const float *__restrict__ table, int table_len,
                                                               float bound, RateTables T, unsigned long long *__restrict__ bits)
{
    extern __shared__ float s_table[];
    __shared__ int s_unsorted;
    __shared__ int2 s_rowinfo[kRateMaxRows];
    __shared__ float s_cand[kRateMaxCand];
    __shared__ unsigned long long s_red[kBlock / kWave][kRateMaxCand];
    const int seg = blockIdx.x / bps, part = blockIdx.x - seg * bps;
    if (threadIdx.x == 0) s_unsorted = 0;
    for (int i = threadIdx.x; i < table_len; i += blockDim.x) s_table[i] = table[i];
    for (int r = threadIdx.x; r < T.rows; r += blockDim.x) s_rowinfo[r] = make_int2(T.offsets[r], T.sizes[r] - 2);
    if (static_cast<int>(threadIdx.x) < n_cand)
        s_cand[threadIdx.x] = cand[(cand_per_image ? static_cast<int64_t>(seg / segs_per_image) * n_cand : 0) + threadIdx.x];
    __syncthreads();
    for (int i = threadIdx.x; i + 1 < table_len; i += blockDim.x)
        if (!(s_table[i] <= s_table[i + 1])) s_unsorted = 1;
    __syncthreads();
    const bool sorted = s_unsorted == 0;
    const float *py = y + static_cast<int64_t>(seg) * per_seg, *ps = scales + static_cast<int64_t>(seg) * per_seg;
    const float *pm = nullptr;
    if constexpr (kMean) {
        const int64_t at = static_cast<int64_t>(seg / segs_per_image) * param_stride + static_cast<int64_t>(seg % segs_per_image) * per_seg;
        ps = scales + at;
        pm = means + at;
    }
    unsigned long long acc[kNC];
#pragma unroll
    for (int k = 0; k < kNC; ++k) acc[k] = 0ull;
    for (int64_t i = static_cast<int64_t>(part) * kBlock + threadIdx.x; i < per_seg; i += static_cast<int64_t>(bps) * kBlock) {
        float yv = py[i];
        if constexpr (kMean) yv = mean_sub(yv, pm[i]);
        const float sb = fmaxf(ps[i], bound);   // LowerBound first, then the step
#pragma unroll
        for (int k = 0; k < kNC; ++k) {
            if (k < n_cand) {
                const float step = s_cand[k];
                const float s = step_div(sb, step);
                int idx;
                if (sorted && s == s) {
                    int lo = 0, hi = table_len - 1;   // first j in [0, len - 1) with table[j] >= s, len - 1 if none
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (s_table[mid] < s) lo = mid + 1; else hi = mid;
                    }
                    idx = lo;
                } else {
                    idx = table_len - 1;
                    for (int j = 0; j < table_len - 1; ++j) idx -= (s <= s_table[j]) ? 1 : 0;
                }
                const float q = round_even(step_div(yv, step));
                acc[k] += symbol_cost(T, s_rowinfo, idx, static_cast<int32_t>(q));
            }
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < kNC; ++k) {
        if (k < n_cand) {
            unsigned long long v = acc[k];
            for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
            if (lane == 0) s_red[wave][k] = v;
        }
    }
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < n_cand) {
        unsigned long long v = 0ull;
        for (int w = 0; w < kBlock / kWave; ++w) v += s_red[w][threadIdx.x];
        atomicAdd(&bits[static_cast<int64_t>(seg) * n_cand + threadIdx.x], v);
    }
}

// pred_bytes(b, k) of the byte bound; one thread per image walks its candidates in order and keeps the first that fits
__global__ void rate_select_kernel(const unsigned long long *__restrict__ bits, int n_images, int segs_per_image, int64_t per_seg,
                                   const float *__restrict__ cand, int n_cand, int cand_per_image, const int32_t *__restrict__ extra_words,
                                   const int64_t *__restrict__ budget, float *__restrict__ steps_out, int32_t *__restrict__ choice,
                                   int64_t *__restrict__ pred_bytes)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_images) return;
    const int64_t extra = extra_words ? 4 * static_cast<int64_t>(extra_words[b]) : 0, want = budget[b];
    int pick = -1;
    int64_t pred = 0;
    for (int k = 0; k < n_cand && pick < 0; ++k) {
        pred = extra;
        for (int l = 0; l < segs_per_image; ++l) {
            const unsigned long long q = bits[(static_cast<int64_t>(b) * segs_per_image + l) * n_cand + k];
            pred += 4 * (2 + static_cast<int64_t>((q + 4ull * static_cast<unsigned long long>(per_seg)) >> 21));
        }
        if (pred <= want) pick = k;
    }
    const int k = pick < 0 ? n_cand - 1 : pick;   // nothing fits: the largest step, whose prediction `pred` holds
    choice[b] = pick < 0 ? (k | BASIC_RATE_NO_FIT) : k;
    steps_out[b] = cand[(cand_per_image ? static_cast<int64_t>(b) * n_cand : 0) + k];
    pred_bytes[b] = pred;
}

// rate_select_kernel for groups of tiles (a tiled picture's budget is one number over all its tiles): workgroup g owns group g, its
// threads stride over the group's tiles with one 64-bit sum per candidate each, the sums meet in the wave (shuffles) and in the
// workgroup (LDS), thread 0 walks the candidates, and every thread writes its tiles' step and prediction at the chosen one.
// Integer sums only: the result depends on neither the block width nor the order.  The plan arrays are the entry point's own
// validated upload.
constexpr int kGroupMaxBlock = 1024;

__device__ __forceinline__ int64_t tile_pred_bytes(const unsigned long long *__restrict__ bits, int first_seg, int lanes, int64_t per_seg,
                                                   int32_t extra_words, int n_cand, int k)
{
    int64_t pred = 4 * static_cast<int64_t>(extra_words);
    for (int l = 0; l < lanes; ++l) {
        const unsigned long long q = bits[static_cast<int64_t>(first_seg + l) * n_cand + k];
        pred += 4 * (2 + static_cast<int64_t>((q + 4ull * static_cast<unsigned long long>(per_seg)) >> 21));
    }
    return pred;
}

template <int kNC>
__global__ __launch_bounds__(kGroupMaxBlock) void rate_select_groups_kernel(
    const unsigned long long *__restrict__ bits, int lanes, const int32_t *__restrict__ tile_first_seg,
    const int64_t *__restrict__ tile_per_seg, const int32_t *__restrict__ tile_extra_words, const int32_t *__restrict__ group_first,
    const int32_t *__restrict__ group_tiles, const float *__restrict__ cand, int n_cand, int cand_per_group,
    const int64_t *__restrict__ budget, float *__restrict__ steps_out, int32_t *__restrict__ choice, int64_t *__restrict__ pred_bytes,
    float *__restrict__ tile_steps, int64_t *__restrict__ tile_pred)
{
    __shared__ long long s_red[kGroupMaxBlock / kWave][kRateMaxCand];
    __shared__ long long s_pred[kRateMaxCand];
    __shared__ int s_pick;
    const int g = blockIdx.x;
    const int t0 = group_first[g], t1 = group_first[g + 1];
    long long acc[kNC];
#pragma unroll
    for (int k = 0; k < kNC; ++k) acc[k] = 0;
    for (int i = t0 + static_cast<int>(threadIdx.x); i < t1; i += static_cast<int>(blockDim.x)) {
        const int t = group_tiles[i];
        const int first = tile_first_seg[t];
        const int64_t per = tile_per_seg[t];
        const int32_t extra = tile_extra_words ? tile_extra_words[t] : 0;
#pragma unroll
        for (int k = 0; k < kNC; ++k)
            if (k < n_cand) acc[k] += tile_pred_bytes(bits, first, lanes, per, extra, n_cand, k);
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, n_waves = (blockDim.x + kWave - 1) / kWave;
#pragma unroll
    for (int k = 0; k < kNC; ++k) {
        if (k < n_cand) {
            long long v = acc[k];
            for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
            if (lane == 0) s_red[wave][k] = v;
        }
    }
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < n_cand) {
        long long v = 0;
        for (int w = 0; w < n_waves; ++w) v += s_red[w][threadIdx.x];
        s_pred[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t want = budget[g];
        int pick = -1;
        for (int k = 0; k < n_cand && pick < 0; ++k)
            if (s_pred[k] <= want) pick = k;
        const int k = pick < 0 ? n_cand - 1 : pick;   // nothing fits: the largest step and its prediction
        choice[g] = pick < 0 ? (k | BASIC_RATE_NO_FIT) : k;
        pred_bytes[g] = s_pred[k];
        s_pick = k;
    }
    __syncthreads();
    const int k = s_pick;
    const float step = cand[(cand_per_group ? static_cast<int64_t>(g) * n_cand : 0) + k];
    if (threadIdx.x == 0) steps_out[g] = step;
    for (int i = t0 + static_cast<int>(threadIdx.x); i < t1; i += static_cast<int>(blockDim.x)) {
        const int t = group_tiles[i];
        tile_steps[t] = step;
        tile_pred[t] = tile_pred_bytes(bits, tile_first_seg[t], lanes, tile_per_seg[t], tile_extra_words ? tile_extra_words[t] : 0, n_cand, k);
    }
}

__global__ void rate_refine_kernel(const float *__restrict__ cand_in, int cand_per_image, int n_cand, const int32_t *__restrict__ choice,
                                   int n_images, const float *__restrict__ t, float *__restrict__ cand_out)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_images * n_cand) return;
    const int b = i / n_cand, j = i - b * n_cand;
    const float *c = cand_in + (cand_per_image ? static_cast<int64_t>(b) * n_cand : 0);
    const int32_t ch = choice[b];
    const int k = clampi(ch & ~BASIC_RATE_NO_FIT, 0, n_cand - 1);
    float v = c[k];
    if (k > 0 && !(ch & BASIC_RATE_NO_FIT) && j < n_cand - 1) {
        // plain operators under the pragma above: three roundings (the *_rn intrinsics are inline functions compiled under the
        // build's own contraction mode, and their multiply and add would fuse here)
        const float lo = c[k - 1], hi = v;
        const float d = hi - lo;
        const float p = d * t[j];
        v = fminf(lo + p, hi);
    }
    cand_out[i] = v;
}

__global__ void eb_quantize_index_kernel(const float *__restrict__ z, const float *__restrict__ medians, int64_t total,
                                         int channels, int hw, int32_t *__restrict__ symbols,
                                         int32_t *__restrict__ indexes, float *__restrict__ zhat)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int c = static_cast<int>((i / hw) % channels);
        const float m = medians[c];
        const float q = round_even(z[i] - m);
        symbols[i] = static_cast<int32_t>(q);
        indexes[i] = c;
        if (zhat) zhat[i] = q + m;
    }
}

__global__ void eb_dequantize_kernel(const int32_t *__restrict__ symbols, const float *__restrict__ medians,
                                     int64_t total, int channels, int hw, float *__restrict__ zhat)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int c = static_cast<int>((i / hw) % channels);
        zhat[i] = static_cast<float>(symbols[i]) + medians[c];
    }
}

__global__ void i32_to_f32_kernel(const int32_t *__restrict__ in, int64_t n, float *__restrict__ out)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x)
        out[i] = static_cast<float>(in[i]);
}

// lane streams of the scan-line coder: both arrays from coding order [B][P][K][L] to one run per lane stream, [B][K][P][L].
// A thread owns an output element: stores are contiguous, loads contiguous in runs of L (>= 16 elements, 64 bytes).
__global__ void lanes_pack_kernel(const int32_t *__restrict__ sym, const int32_t *__restrict__ idx, int64_t total, int positions,
                                  int lanes, int width, int32_t *__restrict__ sym_out, int32_t *__restrict__ idx_out)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t run = i / width;   // (b * K + k) * P + p
        const int l = static_cast<int>(i - run * width);
        const int64_t bk = run / positions;
        const int p = static_cast<int>(run - bk * positions);
        const int64_t b = bk / lanes;
        const int k = static_cast<int>(bk - b * lanes);
        const int64_t src = ((b * positions + p) * lanes + k) * width + l;
        sym_out[i] = sym[src];
        idx_out[i] = idx[src];
    }
}

// lane streams of the group coders (GaussianConditional: one group; topo-group coders: the plan's groups): both arrays from
// group-major coding order [B][n] to one run per lane stream, [B][K][n / K], where stream (b, k) is the concatenation over the
// groups g of the k-th of K equal parts of group g.  bases[0 .. G] are the groups' first elements (bases[G] = n), every group
// a multiple of K long (the caller's rule; an element a broken table would send past the image is left unwritten).  A thread
// owns an output element and finds its group by bisection: stores are contiguous, loads contiguous within a part.
__global__ void group_lanes_pack_kernel(const int32_t *__restrict__ sym, const int32_t *__restrict__ idx, int64_t total, int64_t n,
                                        const int64_t *__restrict__ bases, int groups, int lanes, int32_t *__restrict__ sym_out,
                                        int32_t *__restrict__ idx_out)
{
    const int64_t per = n / lanes;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t b = i / n, r = i - b * n;
        const int64_t k = r / per, o = r - k * per;   // element o of lane stream (b, k)
        const int64_t t = o * lanes;                  // the group holding it is the last one that starts at or before t
        int lo = 0, hi = groups - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (bases[mid] <= t) lo = mid; else hi = mid - 1;
        }
        const int64_t gb = bases[lo], part = (bases[lo + 1] - gb) / lanes;
        const int64_t src = gb + k * part + (o - gb / lanes);
        if (src >= 0 && src < n) {
            sym_out[i] = sym[b * n + src];
            idx_out[i] = idx[b * n + src];
        }
    }
}

// argmin_j |s - table[j]|, first minimum (torch.argmin on CPU returns the first occurrence).
__device__ __forceinline__ int nearest_scale(float s, const float *tab, int n)
{
    int best = 0;
    float bd = fabsf(s - tab[0]);
    for (int j = 1; j < n; ++j) {
        const float d = fabsf(s - tab[j]);
        if (d < bd) { bd = d; best = j; }
    }
    return best;
}

// MODE 0: encode (symbols + indexes + write-back), 1: indexes only, 2: scatter decoded symbols.
template <int MODE>
__global__ void pgm_gauss_group_kernel(const float *__restrict__ y, const float *__restrict__ params, int batch,
                                       int channels, int hw, const int32_t *__restrict__ elems, int64_t n_elems,
                                       const float *__restrict__ table, int table_len, int32_t *symbols,
                                       int32_t *indexes, int64_t per_image, int64_t out_base, float *ybuf)
{
    extern __shared__ float s_table[];
    if (MODE != 2) {
        for (int i = threadIdx.x; i < table_len; i += blockDim.x) s_table[i] = table[i];
        __syncthreads();
    }
    const int64_t total = static_cast<int64_t>(batch) * n_elems;
    const int64_t chw = static_cast<int64_t>(channels) * hw;
    for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total;
         t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t b = t / n_elems, k = t - b * n_elems;
        const int32_t e = elems[k];  // c*hw + p
        const int c = e / hw, p = e - c * hw;
        // split_interleave: channel 2c = mean, 2c+1 = scale (pgm_coder.py:743-752)
        const float *pb = params + (b * 2 * chw) + static_cast<int64_t>(2 * c) * hw + p;
        const float mu = pb[0];
        const int64_t o = b * per_image + out_base + k;
        if (MODE == 0 || MODE == 1) indexes[o] = nearest_scale(pb[hw], s_table, table_len);
        if (MODE == 0) {
            const float q = round_even(y[b * chw + e] - mu);
            symbols[o] = static_cast<int32_t>(q);
            ybuf[b * chw + e] = q + mu;
        }
        if (MODE == 2) ybuf[b * chw + e] = static_cast<float>(symbols[o]) + mu;
    }
}

constexpr int kMseBlock = 1024;
__global__ __launch_bounds__(kMseBlock) void mse_per_image_kernel(const float *__restrict__ a, const float *__restrict__ b, int64_t elems,
                                                                  float *__restrict__ mse)
{
    // one workgroup per image; per thread four independent 16-byte streams (a batch-1 image is 1.2 M elements on ONE compute
    // unit: scalar loads took 1.9 ms per Kodak-shaped image), pairwise tree in LDS; the order is fixed by the shape alone
    __shared__ float red[kMseBlock];
    const int img = blockIdx.x;
    const float *pa = a + static_cast<int64_t>(img) * elems, *pb = b + static_cast<int64_t>(img) * elems;
    float acc = 0.f;
    typedef float f4 __attribute__((ext_vector_type(4)));
    int64_t done = 0;
    if (((reinterpret_cast<uintptr_t>(pa) | reinterpret_cast<uintptr_t>(pb)) & 15u) == 0) {
        const f4 *qa = reinterpret_cast<const f4 *>(pa), *qb = reinterpret_cast<const f4 *>(pb);
        const int64_t n4 = elems >> 2;
        f4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
        int64_t i = threadIdx.x;
        for (; i + 3 * kMseBlock < n4; i += 4 * kMseBlock) {
            const f4 d0 = qa[i] - qb[i], d1 = qa[i + kMseBlock] - qb[i + kMseBlock], d2 = qa[i + 2 * kMseBlock] - qb[i + 2 * kMseBlock],
                     d3 = qa[i + 3 * kMseBlock] - qb[i + 3 * kMseBlock];
            s0 += d0 * d0; s1 += d1 * d1; s2 += d2 * d2; s3 += d3 * d3;
        }
        for (; i < n4; i += kMseBlock) { const f4 d = qa[i] - qb[i]; s0 += d * d; }
        const f4 t = (s0 + s1) + (s2 + s3);
        acc = (t[0] + t[1]) + (t[2] + t[3]);
        done = n4 << 2;
    }
    for (int64_t i = done + threadIdx.x; i < elems; i += kMseBlock) {
        const float d = pa[i] - pb[i];
        acc += d * d;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kMseBlock / 2; s > 0; s >>= 1) {
        if (static_cast<int>(threadIdx.x) < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) mse[img] = red[0] / static_cast<float>(elems);
}

// ---- rate estimate ("prior_entropy", nats per image): -sum log(max(P(q), bound)) -------------------------------
// MODE 0: CompressAI GaussianConditional._likelihood (upstream; call site compressai_coder.py:352-375):
//         zero mean, v = |q|, P = Phi((.5 - v)/s) - Phi((-.5 - v)/s), Phi(t) = .5 erfc(-t/sqrt2), s = max(scale, bound_s)
// MODE 1: PGM coder (pgm_coder.py:374-389,757-778): Normal(mu, max(scale, bound_s)).cdf(q + .5) - cdf(q - .5) with
//         torch's cdf = .5 (1 + erf((x - mu) / (s sqrt2))), params "split_interleave" in a [B][2C][HW] tensor.
template <int MODE>
__global__ void gauss_nll_per_image_kernel(const float *__restrict__ q, const float *__restrict__ scales_or_params,
                                           int64_t elems, int hw, float bound_s, float bound_p, float *__restrict__ nll)
{
    __shared__ float red[kBlock];
    const int img = blockIdx.x;
    const float *pq = q + static_cast<int64_t>(img) * elems;
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < elems; i += blockDim.x) {
        float p;
        if (MODE == 0) {
            const float s = fmaxf(scales_or_params[static_cast<int64_t>(img) * elems + i], bound_s);
            const float v = fabsf(pq[i]);
            const float c = -0.70710678118654752440f;
            p = 0.5f * erfcf(c * ((0.5f - v) / s)) - 0.5f * erfcf(c * ((-0.5f - v) / s));
        } else {
            const int64_t c = i / hw, pos = i - c * hw;
            const float *pp = scales_or_params + static_cast<int64_t>(img) * 2 * elems + (2 * c) * hw + pos;
            const float mu = pp[0], s = fmaxf(pp[hw], bound_s);
            const float r = 0.70710678118654752440f / s;  // 1 / (s sqrt2) as torch: (x - mu) * s.reciprocal() / sqrt2
            if (MODE == 2) {   // likelihood of the ROUNDED RESIDUAL under the zero-mean density (pgm_coder.py:376-387)
                const float v = rintf(pq[i] - mu);
                p = 0.5f * (1.f + erff((v + 0.5f) * r)) - 0.5f * (1.f + erff((v - 0.5f) * r));
            } else {
                p = 0.5f * (1.f + erff((pq[i] + 0.5f - mu) * r)) - 0.5f * (1.f + erff((pq[i] - 0.5f - mu) * r));
            }
        }
        acc += -logf(fmaxf(p, bound_p));
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = kBlock / 2; st > 0; st >>= 1) {
        if (static_cast<int>(threadIdx.x) < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) nll[img] = red[0];
}

// MODE 0 of the kernel above under a quantiser step: q = the coded symbol rint(y / step) as float, its likelihood taken
// under s' = max(scale, bound_s) / step[image] -- what the step coder's tables see.  One workgroup per image: the step is uniform.
__global__ void gauss_nll_per_image_q_kernel(const float *__restrict__ q, const float *__restrict__ scales, int64_t elems,
                                             const float *__restrict__ steps, int n_steps, float bound_s, float bound_p,
                                             float *__restrict__ nll)
{
    __shared__ float red[kBlock];
    const int img = blockIdx.x;
    const float *pq = q + static_cast<int64_t>(img) * elems, *ps = scales + static_cast<int64_t>(img) * elems;
    const float step = steps[n_steps == 1 ? 0 : img];
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < elems; i += blockDim.x) {
        const float s = step_div(fmaxf(ps[i], bound_s), step);
        const float v = fabsf(pq[i]);
        const float c = -0.70710678118654752440f;
        const float p = 0.5f * erfcf(c * ((0.5f - v) / s)) - 0.5f * erfcf(c * ((-0.5f - v) / s));
        acc += -logf(fmaxf(p, bound_p));
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = kBlock / 2; st > 0; st >>= 1) {
        if (static_cast<int>(threadIdx.x) < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) nll[img] = red[0];
}

// EntropyBottleneck likelihood (upstream _logits_cumulative; call site compressai_coder.py:203-228): per channel a
// 1-3-3-3-3-1 network with pre-activated parameters coef[c][58] = softplus(M0[3]) b0[3] tanh(f0)[3] | softplus(M1[9]) b1[3]
// tanh(f1)[3] | M2.. | M3.. | softplus(M4[3]) b4[1].
__device__ __forceinline__ float eb_logits(const float *k, float v)
{
    float h[3], t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { h[i] = k[i] * v + k[3 + i]; h[i] += k[6 + i] * tanhf(h[i]); }
    k += 9;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { t[i] = k[3 * i] * h[0] + k[3 * i + 1] * h[1] + k[3 * i + 2] * h[2] + k[9 + i]; t[i] += k[12 + i] * tanhf(t[i]); }
#pragma unroll
        for (int i = 0; i < 3; ++i) h[i] = t[i];
        k += 15;
    }
    return k[0] * h[0] + k[1] * h[1] + k[2] * h[2] + k[3];
}

__global__ void eb_nll_per_image_kernel(const float *__restrict__ zq, const float *__restrict__ coef, int channels, int hw,
                                        float bound_p, float *__restrict__ nll)
{
    __shared__ float red[kBlock];
    const int img = blockIdx.x;
    const int64_t elems = static_cast<int64_t>(channels) * hw;
    const float *pz = zq + static_cast<int64_t>(img) * elems;
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < elems; i += blockDim.x) {
        const float *k = coef + (i / hw) * 58;
        const float lower = eb_logits(k, pz[i] - 0.5f), upper = eb_logits(k, pz[i] + 0.5f);
        const float sg = (lower + upper) > 0.f ? -1.f : ((lower + upper) < 0.f ? 1.f : 0.f);
        const float p = fabsf(1.f / (1.f + expf(-sg * upper)) - 1.f / (1.f + expf(-sg * lower)));
        acc += -logf(fmaxf(p, bound_p));
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = kBlock / 2; st > 0; st >>= 1) {
        if (static_cast<int>(threadIdx.x) < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) nll[img] = red[0];
}

}  // namespace

extern "C" int basic_gc_quantize_index_dev(const float *d_y, const float *d_scales, int64_t n, const float *d_table,
                                           int table_len, float scale_bound, int32_t *d_symbols, int32_t *d_indexes,
                                           float *d_yhat, void *hip_stream)
{
    BASIC_REQUIRE(d_y && d_scales && d_table && d_symbols && d_indexes && n >= 0 && table_len >= 1 && table_len <= 4096,
                  "gc_quantize_index: bad argument");
    if (n == 0) return BASIC_OK;
    hipLaunchKernelGGL(gc_quantize_index_kernel, dim3(grid_for(n)), dim3(kBlock), table_len * sizeof(float),
                       as_stream(hip_stream), d_y, d_scales, n, d_table, table_len, scale_bound, d_symbols, d_indexes, d_yhat);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_gc_quantize_index_q_dev(const float *d_y, const float *d_scales, int64_t n, int64_t per_image,
                                             const float *d_steps, int n_steps, const float *d_table, int table_len,
                                             float scale_bound, int32_t *d_symbols, int32_t *d_indexes, float *d_yhat,
                                             void *hip_stream)
{
    BASIC_REQUIRE(d_y && d_scales && d_steps && d_table && d_symbols && d_indexes && n >= 0 && table_len >= 1 && table_len <= 4096,
                  "gc_quantize_index_q: bad argument");
    BASIC_REQUIRE(per_image >= 1 && n % per_image == 0 && (n_steps == 1 || n_steps == n / per_image),
                  "gc_quantize_index_q: n is a whole number of images of per_image elements, with one step for all or one each");
    if (n == 0) return BASIC_OK;
    hipLaunchKernelGGL(gc_quantize_index_q_kernel, dim3(grid_for(n)), dim3(kBlock), table_len * sizeof(float), as_stream(hip_stream),
                       d_y, d_scales, n, per_image, d_steps, n_steps, d_table, table_len, scale_bound, d_symbols, d_indexes, d_yhat);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_gc_dequantize_q_dev(const int32_t *d_sym, int64_t n, int64_t per_image, const float *d_steps, int n_steps,
                                         float *d_yhat, void *hip_stream)
{
    BASIC_REQUIRE(d_sym && d_steps && d_yhat && n >= 0, "gc_dequantize_q: bad argument");
    BASIC_REQUIRE(per_image >= 1 && n % per_image == 0 && (n_steps == 1 || n_steps == n / per_image),
                  "gc_dequantize_q: n is a whole number of images of per_image elements, with one step for all or one each");
    if (n == 0) return BASIC_OK;
    hipLaunchKernelGGL(gc_dequantize_q_kernel, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(hip_stream), d_sym, n, per_image, d_steps,
                       n_steps, d_yhat);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_gc_quantize_index_ms_dev(const float *d_y, const float *d_scales, const float *d_means, int64_t n, int64_t per_image,
                                              int64_t param_stride, const float *d_steps, int n_steps, const float *d_table,
                                              int table_len, float scale_bound, int32_t *d_symbols, int32_t *d_indexes, float *d_yhat,
                                              void *hip_stream)
{
    BASIC_REQUIRE(d_scales && d_table && d_indexes && n >= 0 && table_len >= 1 && table_len <= 4096, "gc_quantize_index_ms: bad argument");
    BASIC_REQUIRE(d_y ? (d_symbols && d_means) : (!d_symbols && !d_yhat),
                  "gc_quantize_index_ms: d_y needs d_means and d_symbols; without d_y (indexes only) there is neither d_symbols nor d_yhat");
    if (!d_steps) n_steps = 0;
    BASIC_REQUIRE(per_image >= 1 && n % per_image == 0 && (n_steps == 0 || n_steps == 1 || n_steps == n / per_image),
                  "gc_quantize_index_ms: n is a whole number of images of per_image elements, with no step, one for all or one each");
    BASIC_REQUIRE(param_stride >= per_image, "gc_quantize_index_ms: param_stride is at least per_image");
    if (n == 0) return BASIC_OK;
    const dim3 grid(grid_for(n)), block(kBlock);
    const size_t lds = table_len * sizeof(float);
    if (n_steps)
        hipLaunchKernelGGL(gc_quantize_index_ms_kernel<true>, grid, block, lds, as_stream(hip_stream), d_y, d_scales, d_means, n, per_image,
                           param_stride, d_steps, n_steps, d_table, table_len, scale_bound, d_symbols, d_indexes, d_yhat);
    else
        hipLaunchKernelGGL(gc_quantize_index_ms_kernel<false>, grid, block, lds, as_stream(hip_stream), d_y, d_scales, d_means, n, per_image,
                           param_stride, d_steps, n_steps, d_table, table_len, scale_bound, d_symbols, d_indexes, d_yhat);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_gc_dequantize_ms_dev(const int32_t *d_sym, const float *d_means, int64_t n, int64_t per_image, int64_t param_stride,
                                          const float *d_steps, int n_steps, float *d_yhat, void *hip_stream)
{
    BASIC_REQUIRE(d_sym && d_means && d_yhat && n >= 0, "gc_dequantize_ms: bad argument");
    if (!d_steps) n_steps = 0;
    BASIC_REQUIRE(per_image >= 1 && n % per_image == 0 && (n_steps == 0 || n_steps == 1 || n_steps == n / per_image),
                  "gc_dequantize_ms: n is a whole number of images of per_image elements, with no step, one for all or one each");
    BASIC_REQUIRE(param_stride >= per_image, "gc_dequantize_ms: param_stride is at least per_image");
    if (n == 0) return BASIC_OK;
    if (n_steps)
        hipLaunchKernelGGL(gc_dequantize_ms_kernel<true>, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(hip_stream), d_sym, d_means, n,
                           per_image, param_stride, d_steps, n_steps, d_yhat);
    else
        hipLaunchKernelGGL(gc_dequantize_ms_kernel<false>, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(hip_stream), d_sym, d_means, n,
                           per_image, param_stride, d_steps, n_steps, d_yhat);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

namespace {

// both rate-curve entry points: d_means == nullptr is the zero-mean coder (param_stride unused)
int rate_curve_launch(const float *d_y, const float *d_scales, const float *d_means, int64_t param_stride, int n_seg, int64_t per_seg,
                      int segs_per_image, const float *d_cand, int n_cand, int cand_per_image, const float *d_table, int table_len,
                      float scale_bound, const basic_rans_tables *t, uint64_t *d_bits, void *hip_stream)
{
    BASIC_REQUIRE(d_y && d_scales && d_cand && d_table && t && d_bits && table_len >= 1 && table_len <= 4096, "gc_rate_curve: bad argument");
    BASIC_REQUIRE(n_seg >= 1 && per_seg >= 1 && segs_per_image >= 1 && n_seg % segs_per_image == 0,
                  "gc_rate_curve: n_seg is a whole number of images of segs_per_image segments, per_seg >= 1");
    BASIC_REQUIRE(n_cand >= 1 && n_cand <= kRateMaxCand && (cand_per_image == 0 || cand_per_image == 1),
                  "gc_rate_curve: 1 to 32 candidates, shared (0) or one set per image (1)");
    BASIC_REQUIRE(per_seg <= (INT64_MAX >> 22), "gc_rate_curve: per_seg * 2^22 does not fit 63 bits");
    RansRateView v;
    int rc = rans_rate_view(t, &v);
    if (rc) return rc;
    BASIC_REQUIRE(v.bypass && v.precision == 16 && v.rows <= kRateMaxRows,
                  "gc_rate_curve: the table set must code with bypass, at precision 16, in at most 1024 rows");
    const hipStream_t st = as_stream(hip_stream);
    BASIC_HIP_TRY(hipMemsetAsync(d_bits, 0, sizeof(uint64_t) * static_cast<size_t>(n_seg) * n_cand, st));
    // workgroups per segment: four elements a thread when the segment is long enough, and a grid of about 16 K workgroups at most
    int64_t bps = (per_seg + 4 * kBlock - 1) / (4 * kBlock);
    const int64_t cap = n_seg >= 16384 ? 1 : 16384 / n_seg;
    if (bps > cap) bps = cap;
    const RateTables T{v.cost, v.sizes, v.offsets, v.rows, v.stride, static_cast<uint32_t>(v.bypass_precision)};
    const dim3 grid(static_cast<unsigned>(n_seg * bps)), block(kBlock);
    const size_t lds = table_len * sizeof(float);
    auto *bits = reinterpret_cast<unsigned long long *>(d_bits);
#define BASIC_RATE_LAUNCH(NC, MEAN)                                                                                                   \
    hipLaunchKernelGGL((gc_rate_curve_kernel<NC, MEAN>), grid, block, lds, st, d_y, d_scales, d_means, param_stride, per_seg,         \
                       segs_per_image, static_cast<int>(bps), d_cand, n_cand, cand_per_image, d_table, table_len, scale_bound, T, bits)
    if (d_means) {
        if (n_cand <= 2) BASIC_RATE_LAUNCH(2, true);
        else if (n_cand <= 8) BASIC_RATE_LAUNCH(8, true);
        else if (n_cand <= 16) BASIC_RATE_LAUNCH(16, true);
        else BASIC_RATE_LAUNCH(32, true);
    } else {
        if (n_cand <= 2) BASIC_RATE_LAUNCH(2, false);
        else if (n_cand <= 8) BASIC_RATE_LAUNCH(8, false);
        else if (n_cand <= 16) BASIC_RATE_LAUNCH(16, false);
        else BASIC_RATE_LAUNCH(32, false);
    }
#undef BASIC_RATE_LAUNCH
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

}  // namespace

extern "C" int basic_gc_rate_curve_dev(const float *d_y, const float *d_scales, int n_seg, int64_t per_seg, int segs_per_image,
                                       const float *d_cand, int n_cand, int cand_per_image, const float *d_table, int table_len,
                                       float scale_bound, const basic_rans_tables *t, uint64_t *d_bits, void *hip_stream)
{
    return rate_curve_launch(d_y, d_scales, nullptr, 0, n_seg, per_seg, segs_per_image, d_cand, n_cand, cand_per_image, d_table, table_len,
                             scale_bound, t, d_bits, hip_stream);
}

extern "C" int basic_gc_rate_curve_ms_dev(const float *d_y, const float *d_scales, const float *d_means, int64_t param_stride, int n_seg,
                                          int64_t per_seg, int segs_per_image, const float *d_cand, int n_cand, int cand_per_image,
                                          const float *d_table, int table_len, float scale_bound, const basic_rans_tables *t,
                                          uint64_t *d_bits, void *hip_stream)
{
    BASIC_REQUIRE(d_means, "gc_rate_curve_ms: d_means is null");
    BASIC_REQUIRE(per_seg >= 1 && per_seg <= (INT64_MAX >> 32) && segs_per_image >= 1 && param_stride >= per_seg * segs_per_image,
                  "gc_rate_curve_ms: param_stride is at least the per_seg * segs_per_image elements of an image");
    return rate_curve_launch(d_y, d_scales, d_means, param_stride, n_seg, per_seg, segs_per_image, d_cand, n_cand, cand_per_image, d_table,
                             table_len, scale_bound, t, d_bits, hip_stream);
}

extern "C" int basic_rate_select_dev(const uint64_t *d_bits, int n_images, int segs_per_image, int64_t per_seg, const float *d_cand,
                                     int n_cand, int cand_per_image, const int32_t *d_extra_words, const int64_t *d_budget,
                                     float *d_steps_out, int32_t *d_choice, int64_t *d_pred_bytes, void *hip_stream)
{
    BASIC_REQUIRE(d_bits && d_cand && d_budget && d_steps_out && d_choice && d_pred_bytes && n_images >= 1 && segs_per_image >= 1 &&
                      per_seg >= 1 && per_seg <= (INT64_MAX >> 22),
                  "rate_select: bad argument");
    BASIC_REQUIRE(n_cand >= 1 && n_cand <= kRateMaxCand && (cand_per_image == 0 || cand_per_image == 1),
                  "rate_select: 1 to 32 candidates, shared (0) or one set per image (1)");
    hipLaunchKernelGGL(rate_select_kernel, dim3((n_images + kWave - 1) / kWave), dim3(kWave), 0, as_stream(hip_stream),
                       reinterpret_cast<const unsigned long long *>(d_bits), n_images, segs_per_image, per_seg, d_cand, n_cand,
                       cand_per_image, d_extra_words, d_budget, d_steps_out, d_choice, d_pred_bytes);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_rate_select_groups_dev(const uint64_t *d_bits, int n_seg, int lanes, int n_tiles, const int32_t *host_tile_first_seg,
                                            const int64_t *host_tile_per_seg, const int32_t *d_tile_extra_words, int n_groups,
                                            const int32_t *host_group_first, const int32_t *host_group_tiles, void *d_plan,
                                            const float *d_cand, int n_cand, int cand_per_group, const int64_t *d_budget,
                                            float *d_steps_out, int32_t *d_choice, int64_t *d_pred_bytes, float *d_tile_steps,
                                            int64_t *d_tile_pred, int block_threads, void *hip_stream)
{
    BASIC_REQUIRE(d_bits && host_tile_first_seg && host_tile_per_seg && host_group_first && host_group_tiles && d_plan && d_cand &&
                      d_budget && d_steps_out && d_choice && d_pred_bytes && d_tile_steps && d_tile_pred,
                  "rate_select_groups: a null pointer");
    BASIC_REQUIRE(reinterpret_cast<uintptr_t>(d_plan) % sizeof(int64_t) == 0, "rate_select_groups: d_plan must be 8-byte aligned");
    BASIC_REQUIRE(n_seg >= 1 && lanes >= 1 && n_tiles >= 1 && n_groups >= 1, "rate_select_groups: n_seg, lanes, n_tiles and n_groups are >= 1");
    BASIC_REQUIRE(n_cand >= 1 && n_cand <= kRateMaxCand && (cand_per_group == 0 || cand_per_group == 1),
                  "rate_select_groups: 1 to 32 candidates, shared (0) or one set per group (1)");
    if (block_threads == 0) block_threads = kBlock;
    BASIC_REQUIRE(block_threads >= kWave && block_threads <= kGroupMaxBlock && block_threads % kWave == 0,
                  "rate_select_groups: block_threads is 0 (the default) or a multiple of 64 in [64, 1024]");
    for (int t = 0; t < n_tiles; ++t) {
        BASIC_REQUIRE(host_tile_first_seg[t] >= 0 && static_cast<int64_t>(host_tile_first_seg[t]) + lanes <= n_seg,
                      "rate_select_groups: a tile's segments leave the curve tensor");
        BASIC_REQUIRE(host_tile_per_seg[t] >= 1 && host_tile_per_seg[t] <= (INT64_MAX >> 22), "rate_select_groups: a tile's per_seg is out of range");
    }
    BASIC_REQUIRE(host_group_first[0] == 0 && host_group_first[n_groups] <= n_tiles, "rate_select_groups: group_first starts at 0 and lists at most n_tiles");
    for (int g = 0; g < n_groups; ++g)
        BASIC_REQUIRE(host_group_first[g + 1] > host_group_first[g], "rate_select_groups: an empty group");
    const int listed = host_group_first[n_groups];
    std::string seen(static_cast<size_t>(n_tiles), '\0');
    for (int i = 0; i < listed; ++i) {
        const int t = host_group_tiles[i];
        BASIC_REQUIRE(t >= 0 && t < n_tiles, "rate_select_groups: a tile index out of range");
        BASIC_REQUIRE(!seen[t], "rate_select_groups: a tile listed twice");
        seen[t] = 1;
    }
    // the plan as the kernel reads it: int64 per_seg [T] | int32 first_seg [T] | int32 group_first [G + 1] | int32 group_tiles [listed]
    const hipStream_t st = as_stream(hip_stream);
    char *plan = static_cast<char *>(d_plan);
    const size_t o_first = sizeof(int64_t) * n_tiles, o_gfirst = o_first + sizeof(int32_t) * n_tiles,
                 o_gtiles = o_gfirst + sizeof(int32_t) * (n_groups + 1);
    BASIC_HIP_TRY(hipMemcpyAsync(plan, host_tile_per_seg, sizeof(int64_t) * n_tiles, hipMemcpyHostToDevice, st));
    BASIC_HIP_TRY(hipMemcpyAsync(plan + o_first, host_tile_first_seg, sizeof(int32_t) * n_tiles, hipMemcpyHostToDevice, st));
    BASIC_HIP_TRY(hipMemcpyAsync(plan + o_gfirst, host_group_first, sizeof(int32_t) * (n_groups + 1), hipMemcpyHostToDevice, st));
    BASIC_HIP_TRY(hipMemcpyAsync(plan + o_gtiles, host_group_tiles, sizeof(int32_t) * listed, hipMemcpyHostToDevice, st));
    const dim3 grid(static_cast<unsigned>(n_groups)), block(static_cast<unsigned>(block_threads));
#define BASIC_GROUPS_LAUNCH(NC)                                                                                                          \
    hipLaunchKernelGGL(rate_select_groups_kernel<NC>, grid, block, 0, st, reinterpret_cast<const unsigned long long *>(d_bits), lanes,     \
                       reinterpret_cast<const int32_t *>(plan + o_first), reinterpret_cast<const int64_t *>(plan), d_tile_extra_words,    \
                       reinterpret_cast<const int32_t *>(plan + o_gfirst), reinterpret_cast<const int32_t *>(plan + o_gtiles), d_cand,    \
                       n_cand, cand_per_group, d_budget, d_steps_out, d_choice, d_pred_bytes, d_tile_steps, d_tile_pred)
    if (n_cand <= 2) BASIC_GROUPS_LAUNCH(2);
    else if (n_cand <= 8) BASIC_GROUPS_LAUNCH(8);
    else if (n_cand <= 16) BASIC_GROUPS_LAUNCH(16);
    else BASIC_GROUPS_LAUNCH(32);
#undef BASIC_GROUPS_LAUNCH
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_rate_refine_dev(const float *d_cand_in, int cand_per_image, int n_cand, const int32_t *d_choice, int n_images,
                                     const float *d_t, float *d_cand_out, void *hip_stream)
{
    BASIC_REQUIRE(d_cand_in && d_choice && d_t && d_cand_out && n_images >= 1 && d_cand_out != d_cand_in, "rate_refine: bad argument (out of place)");
    BASIC_REQUIRE(n_cand >= 1 && n_cand <= kRateMaxCand && (cand_per_image == 0 || cand_per_image == 1),
                  "rate_refine: 1 to 32 candidates, shared (0) or one set per image (1)");
    const int total = n_images * n_cand;
    hipLaunchKernelGGL(rate_refine_kernel, dim3((total + kBlock - 1) / kBlock), dim3(kBlock), 0, as_stream(hip_stream), d_cand_in,
                       cand_per_image, n_cand, d_choice, n_images, d_t, d_cand_out);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_eb_quantize_index_dev(const float *d_z, const float *d_medians, int batch, int channels, int hw,
                                           int32_t *d_symbols, int32_t *d_indexes, float *d_zhat, void *hip_stream)
{
    BASIC_REQUIRE(d_z && d_medians && d_symbols && d_indexes && batch >= 1 && channels >= 1 && hw >= 1,
                  "eb_quantize_index: bad argument");
    const int64_t total = static_cast<int64_t>(batch) * channels * hw;
    hipLaunchKernelGGL(eb_quantize_index_kernel, dim3(grid_for(total)), dim3(kBlock), 0, as_stream(hip_stream), d_z,
                       d_medians, total, channels, hw, d_symbols, d_indexes, d_zhat);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_eb_dequantize_dev(const int32_t *d_symbols, const float *d_medians, int batch, int channels,
                                       int hw, float *d_zhat, void *hip_stream)
{
    BASIC_REQUIRE(d_symbols && d_medians && d_zhat && batch >= 1 && channels >= 1 && hw >= 1, "eb_dequantize: bad argument");
    const int64_t total = static_cast<int64_t>(batch) * channels * hw;
    hipLaunchKernelGGL(eb_dequantize_kernel, dim3(grid_for(total)), dim3(kBlock), 0, as_stream(hip_stream), d_symbols,
                       d_medians, total, channels, hw, d_zhat);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_i32_to_f32_dev(const int32_t *d_in, int64_t n, float *d_out, void *hip_stream)
{
    BASIC_REQUIRE(d_in && d_out && n >= 0, "i32_to_f32: bad argument");
    if (n == 0) return BASIC_OK;
    hipLaunchKernelGGL(i32_to_f32_kernel, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(hip_stream), d_in, n, d_out);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_lanes_pack_dev(const int32_t *d_sym, const int32_t *d_idx, int batch, int positions, int channels, int lanes,
                                    int32_t *d_sym_out, int32_t *d_idx_out, void *hip_stream)
{
    BASIC_REQUIRE(d_sym && d_idx && d_sym_out && d_idx_out && batch >= 1 && positions >= 1 && channels >= 1 && lanes >= 1 &&
                      channels % lanes == 0 && d_sym_out != d_sym && d_idx_out != d_idx,
                  "lanes_pack: bad argument");
    const int64_t total = static_cast<int64_t>(batch) * positions * channels;
    hipLaunchKernelGGL(lanes_pack_kernel, dim3(grid_for(total)), dim3(kBlock), 0, as_stream(hip_stream), d_sym, d_idx, total, positions,
                       lanes, channels / lanes, d_sym_out, d_idx_out);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_group_lanes_pack_dev(const int32_t *d_sym, const int32_t *d_idx, int batch, int64_t n, const int64_t *d_bases,
                                          int groups, int lanes, int32_t *d_sym_out, int32_t *d_idx_out, void *hip_stream)
{
    BASIC_REQUIRE(d_sym && d_idx && d_bases && d_sym_out && d_idx_out && batch >= 1 && n >= 1 && groups >= 1 && lanes >= 1 &&
                      lanes <= 256 && n % lanes == 0 && d_sym_out != d_sym && d_idx_out != d_idx,
                  "group_lanes_pack: bad argument (lanes in [1, 256] must divide n; out of place)");
    const int64_t total = static_cast<int64_t>(batch) * n;
    hipLaunchKernelGGL(group_lanes_pack_kernel, dim3(grid_for(total)), dim3(kBlock), 0, as_stream(hip_stream), d_sym, d_idx, total, n,
                       d_bases, groups, lanes, d_sym_out, d_idx_out);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_pgm_gauss_encode_group_dev(const float *d_y, const float *d_params, int batch, int channels,
                                                int hw, const int32_t *d_elems, int64_t n_elems, const float *d_table,
                                                int table_len, int32_t *d_symbols, int32_t *d_indexes,
                                                int64_t per_image, int64_t out_base, float *d_ybuf, void *hip_stream)
{
    BASIC_REQUIRE(d_y && d_params && d_elems && d_table && d_symbols && d_indexes && d_ybuf && batch >= 1 &&
                      channels >= 1 && hw >= 1 && n_elems >= 0 && table_len >= 1 && table_len <= 4096,
                  "pgm_gauss_encode_group: bad argument");
    if (n_elems == 0) return BASIC_OK;
    hipLaunchKernelGGL(pgm_gauss_group_kernel<0>, dim3(grid_for(batch * n_elems)), dim3(kBlock),
                       table_len * sizeof(float), as_stream(hip_stream), d_y, d_params, batch, channels, hw, d_elems,
                       n_elems, d_table, table_len, d_symbols, d_indexes, per_image, out_base, d_ybuf);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_pgm_gauss_index_group_dev(const float *d_params, int batch, int channels, int hw,
                                               const int32_t *d_elems, int64_t n_elems, const float *d_table,
                                               int table_len, int32_t *d_indexes, int64_t per_image, int64_t out_base,
                                               void *hip_stream)
{
    BASIC_REQUIRE(d_params && d_elems && d_table && d_indexes && batch >= 1 && channels >= 1 && hw >= 1 &&
                      n_elems >= 0 && table_len >= 1 && table_len <= 4096,
                  "pgm_gauss_index_group: bad argument");
    if (n_elems == 0) return BASIC_OK;
    hipLaunchKernelGGL(pgm_gauss_group_kernel<1>, dim3(grid_for(batch * n_elems)), dim3(kBlock),
                       table_len * sizeof(float), as_stream(hip_stream), nullptr, d_params, batch, channels, hw,
                       d_elems, n_elems, d_table, table_len, nullptr, d_indexes, per_image, out_base, nullptr);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_pgm_gauss_scatter_group_dev(const int32_t *d_symbols, const float *d_params, int batch,
                                                 int channels, int hw, const int32_t *d_elems, int64_t n_elems,
                                                 int64_t per_image, int64_t in_base, float *d_ybuf, void *hip_stream)
{
    BASIC_REQUIRE(d_symbols && d_params && d_elems && d_ybuf && batch >= 1 && channels >= 1 && hw >= 1 && n_elems >= 0,
                  "pgm_gauss_scatter_group: bad argument");
    if (n_elems == 0) return BASIC_OK;
    hipLaunchKernelGGL(pgm_gauss_group_kernel<2>, dim3(grid_for(batch * n_elems)), dim3(kBlock), 0,
                       as_stream(hip_stream), nullptr, d_params, batch, channels, hw, d_elems, n_elems, nullptr, 0,
                       const_cast<int32_t *>(d_symbols), nullptr, per_image, in_base, d_ybuf);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_mse_per_image_dev(const float *d_a, const float *d_b, int batch, int64_t elems_per_image,
                                       float *d_mse, void *hip_stream)
{
    BASIC_REQUIRE(d_a && d_b && d_mse && batch >= 1 && elems_per_image >= 1, "mse_per_image: bad argument");
    hipLaunchKernelGGL(mse_per_image_kernel, dim3(batch), dim3(kMseBlock), 0, as_stream(hip_stream), d_a, d_b,
                       elems_per_image, d_mse);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_gauss_nll_per_image_dev(const float *d_q, const float *d_scales_or_params, int batch, int channels, int hw,
                                             int interleaved_mean_scale, float scale_bound, float likelihood_bound, float *d_nll,
                                             void *hip_stream)
{
    BASIC_REQUIRE(d_q && d_scales_or_params && d_nll && batch >= 1 && channels >= 1 && hw >= 1, "gauss_nll_per_image: bad argument");
    const int64_t elems = static_cast<int64_t>(channels) * hw;
    if (interleaved_mean_scale == 2)
        hipLaunchKernelGGL(gauss_nll_per_image_kernel<2>, dim3(batch), dim3(kBlock), 0, as_stream(hip_stream), d_q, d_scales_or_params,
                           elems, hw, scale_bound, likelihood_bound, d_nll);
    else if (interleaved_mean_scale)
        hipLaunchKernelGGL(gauss_nll_per_image_kernel<1>, dim3(batch), dim3(kBlock), 0, as_stream(hip_stream), d_q, d_scales_or_params,
                           elems, hw, scale_bound, likelihood_bound, d_nll);
    else
        hipLaunchKernelGGL(gauss_nll_per_image_kernel<0>, dim3(batch), dim3(kBlock), 0, as_stream(hip_stream), d_q, d_scales_or_params,
                           elems, hw, scale_bound, likelihood_bound, d_nll);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_gauss_nll_per_image_q_dev(const float *d_q, const float *d_scales, int batch, int channels, int hw,
                                               const float *d_steps, int n_steps, float scale_bound, float likelihood_bound,
                                               float *d_nll, void *hip_stream)
{
    BASIC_REQUIRE(d_q && d_scales && d_steps && d_nll && batch >= 1 && channels >= 1 && hw >= 1, "gauss_nll_per_image_q: bad argument");
    BASIC_REQUIRE(n_steps == 1 || n_steps == batch, "gauss_nll_per_image_q: one step for all images or one each");
    hipLaunchKernelGGL(gauss_nll_per_image_q_kernel, dim3(batch), dim3(kBlock), 0, as_stream(hip_stream), d_q, d_scales,
                       static_cast<int64_t>(channels) * hw, d_steps, n_steps, scale_bound, likelihood_bound, d_nll);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_eb_nll_per_image_dev(const float *d_zq, const float *d_coef, int batch, int channels, int hw,
                                          float likelihood_bound, float *d_nll, void *hip_stream)
{
    BASIC_REQUIRE(d_zq && d_coef && d_nll && batch >= 1 && channels >= 1 && hw >= 1, "eb_nll_per_image: bad argument");
    hipLaunchKernelGGL(eb_nll_per_image_kernel, dim3(batch), dim3(kBlock), 0, as_stream(hip_stream), d_zq, d_coef, channels, hw,
                       likelihood_bound, d_nll);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

// ---- skip coding (include/basic_hip.h, "Skip coding"): order-preserving compaction of the elements whose table row is at least
// skip_rows, per stream, and its inverse.  A workgroup owns one chunk of BASIC_SKIP_CHUNK elements of one stream, a lane four
// consecutive ones (one 16-byte load where they are aligned and inside the stream; the same lines serve a tail and an unaligned
// stream element by element).  Three launches: the chunks' counts, ONE workgroup's exclusive scan of them in int64 (a chunk's
// base is global: the streams lie back to back in the output, so it already holds the stream's segment start), and the scatter.
// Inside a chunk a kept element's rank is: the kept elements of lower lanes of its wave (four ballots, popcounts under the lane's
// mask) + its own lane's earlier ones + the totals of the lower waves (LDS).  Nothing waits on another workgroup and no atomic
// decides a position.
namespace {

constexpr int kSkipBlock = 256, kSkipLane = 4, kSkipWaves = kSkipBlock / kWave, kSkipScanBlock = 1024;
static_assert(kSkipBlock * kSkipLane == BASIC_SKIP_CHUNK, "a workgroup pass is one chunk");

// the lane's four elements of a stream of `per` elements from `off` on; past the stream's end: 0 (never kept, see skip_keep)
__device__ __forceinline__ void skip_load4(const int32_t *__restrict__ p, int64_t off, int64_t per, int32_t v[kSkipLane])
{
    if (off + kSkipLane <= per && (reinterpret_cast<uintptr_t>(p + off) & 15u) == 0) {
        const int4 q = *reinterpret_cast<const int4 *>(p + off);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < kSkipLane; ++j) v[j] = off + j < per ? p[off + j] : 0;
    }
}

__device__ __forceinline__ void skip_keep(const int32_t v[kSkipLane], int64_t off, int64_t per, int skip_rows, bool keep[kSkipLane])
{
#pragma unroll
    for (int j = 0; j < kSkipLane; ++j) keep[j] = off + j < per && v[j] >= skip_rows;
}

// -> the number of kept elements before the lane's first one inside its chunk; *chunk_total (optional) = the chunk's count.
// s_w: kSkipWaves ints of LDS.  Every thread of the workgroup calls it.
__device__ __forceinline__ int skip_rank(const bool keep[kSkipLane], int *s_w, int *chunk_total)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const unsigned long long below = (1ull << lane) - 1ull;
    int before = 0, total = 0;
#pragma unroll
    for (int j = 0; j < kSkipLane; ++j) {
        const unsigned long long m = __ballot(keep[j]);
        before += __popcll(m & below);
        total += __popcll(m);
    }
    if (lane == 0) s_w[wave] = total;
    __syncthreads();
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kSkipWaves; ++w) {
        if (w < wave) before += s_w[w];
        sum += s_w[w];
    }
    if (chunk_total) *chunk_total = sum;
    return before;
}

__global__ __launch_bounds__(kSkipBlock) void skip_count_kernel(const int32_t *__restrict__ idx, int64_t per, int cps, int skip_rows,
                                                                int64_t *__restrict__ counts)
{
    __shared__ int s_w[kSkipWaves];
    const int64_t s = blockIdx.x / cps;
    const int64_t off = static_cast<int64_t>(blockIdx.x - s * cps) * BASIC_SKIP_CHUNK + threadIdx.x * kSkipLane;
    int32_t v[kSkipLane];
    bool keep[kSkipLane];
    skip_load4(idx + s * per, off, per, v);
    skip_keep(v, off, per, skip_rows, keep);
    int total;
    skip_rank(keep, s_w, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts[0 .. n) -> their exclusive prefix sums, in place; seg (optional) [nstreams + 1]: the base of every stream's first chunk and
// the grand total.  One workgroup, kSkipScanBlock entries a round with the carry in a register of every thread.
__global__ __launch_bounds__(kSkipScanBlock) void skip_scan_kernel(int64_t *__restrict__ counts, int64_t n, int cps, int64_t *__restrict__ seg,
                                                                   int nstreams)
{
    __shared__ long long s_w[kSkipScanBlock / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    long long carry = 0;
    for (int64_t base = 0; base < n; base += kSkipScanBlock) {
        const int64_t i = base + threadIdx.x;
        const long long v = i < n ? counts[i] : 0;
        long long inc = v;
        for (int d = 1; d < kWave; d <<= 1) {
            const long long up = __shfl_up(inc, d, kWave);
            if (lane >= d) inc += up;
        }
        if (lane == kWave - 1) s_w[wave] = inc;
        __syncthreads();
        long long wbase = 0, round = 0;
        for (int w = 0; w < kSkipScanBlock / kWave; ++w) {
            if (w < wave) wbase += s_w[w];
            round += s_w[w];
        }
        const long long excl = carry + wbase + inc - v;
        if (i < n) {
            counts[i] = excl;
            if (seg && i % cps == 0) seg[i / cps] = excl;
        }
        carry += round;
        __syncthreads();   // s_w is rewritten by the next round
    }
    if (seg && threadIdx.x == 0) seg[nstreams] = carry;
}

template <bool kSym>
__global__ __launch_bounds__(kSkipBlock) void skip_scatter_kernel(const int32_t *__restrict__ sym, const int32_t *__restrict__ idx, int64_t per,
                                                                  int cps, int skip_rows, const int64_t *__restrict__ bases,
                                                                  int32_t *__restrict__ sym_out, int32_t *__restrict__ idx_out)
{
    __shared__ int s_w[kSkipWaves];
    const int64_t s = blockIdx.x / cps;
    const int64_t off = static_cast<int64_t>(blockIdx.x - s * cps) * BASIC_SKIP_CHUNK + threadIdx.x * kSkipLane;
    int32_t v[kSkipLane], u[kSkipLane];
    bool keep[kSkipLane];
    skip_load4(idx + s * per, off, per, v);
    if constexpr (kSym) skip_load4(sym + s * per, off, per, u);
    skip_keep(v, off, per, skip_rows, keep);
    int64_t o = bases[blockIdx.x] + skip_rank(keep, s_w, nullptr);   // < the total kept <= nstreams * per
#pragma unroll
    for (int j = 0; j < kSkipLane; ++j) {
        if (keep[j]) {
            idx_out[o] = v[j];
            if constexpr (kSym) sym_out[o] = u[j];
            ++o;
        }
    }
}

__global__ __launch_bounds__(kSkipBlock) void skip_expand_kernel(const int32_t *__restrict__ compact, const int32_t *__restrict__ idx, int64_t per,
                                                                 int cps, int skip_rows, const int64_t *__restrict__ bases,
                                                                 int32_t *__restrict__ dense)
{
    __shared__ int s_w[kSkipWaves];
    const int64_t s = blockIdx.x / cps;
    const int64_t off = static_cast<int64_t>(blockIdx.x - s * cps) * BASIC_SKIP_CHUNK + threadIdx.x * kSkipLane;
    int32_t v[kSkipLane], u[kSkipLane];
    bool keep[kSkipLane];
    skip_load4(idx + s * per, off, per, v);
    skip_keep(v, off, per, skip_rows, keep);
    int64_t o = bases[blockIdx.x] + skip_rank(keep, s_w, nullptr);
#pragma unroll
    for (int j = 0; j < kSkipLane; ++j) u[j] = keep[j] ? compact[o++] : 0;   // keep[j] holds only inside the stream
    int32_t *q = dense + s * per;
    if (off + kSkipLane <= per && (reinterpret_cast<uintptr_t>(q + off) & 15u) == 0) {
        *reinterpret_cast<int4 *>(q + off) = make_int4(u[0], u[1], u[2], u[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kSkipLane; ++j)
            if (off + j < per) q[off + j] = u[j];
    }
}

// the arguments both entry points share; *cps = chunks per stream, *nchunks = the grid
int skip_plan(const void *d_idx, int nstreams, int64_t per, int skip_rows, const void *d_scratch, int *cps, int *nchunks)
{
    BASIC_REQUIRE(d_idx && d_scratch && nstreams >= 1 && per >= 1 && skip_rows >= 0, "skip: bad argument");
    BASIC_REQUIRE(reinterpret_cast<uintptr_t>(d_scratch) % sizeof(int64_t) == 0, "skip: d_scratch must be 8-byte aligned");
    const int64_t c = (per + BASIC_SKIP_CHUNK - 1) / BASIC_SKIP_CHUNK;
    BASIC_REQUIRE(c <= (1ll << 30) && c * nstreams <= (1ll << 30), "skip: more than 2^30 chunks");
    *cps = static_cast<int>(c);
    *nchunks = static_cast<int>(c * nstreams);
    return BASIC_OK;
}

}  // namespace

extern "C" int basic_skip_compact_dev(const int32_t *d_sym, const int32_t *d_idx, int nstreams, int64_t per, int skip_rows, void *d_scratch,
                                      int32_t *d_sym_out, int32_t *d_idx_out, int64_t *d_seg, void *hip_stream)
{
    BASIC_REQUIRE(d_idx_out && d_seg && (d_sym != nullptr) == (d_sym_out != nullptr),
                  "skip_compact: d_idx_out and d_seg are required, d_sym and d_sym_out come together or not at all");
    BASIC_REQUIRE(d_idx_out != d_idx && (!d_sym || d_sym_out != d_sym), "skip_compact: out of place");
    int cps = 0, nchunks = 0;
    const int rc = skip_plan(d_idx, nstreams, per, skip_rows, d_scratch, &cps, &nchunks);
    if (rc) return rc;
    const hipStream_t st = as_stream(hip_stream);
    int64_t *bases = static_cast<int64_t *>(d_scratch);
    hipLaunchKernelGGL(skip_count_kernel, dim3(nchunks), dim3(kSkipBlock), 0, st, d_idx, per, cps, skip_rows, bases);
    hipLaunchKernelGGL(skip_scan_kernel, dim3(1), dim3(kSkipScanBlock), 0, st, bases, static_cast<int64_t>(nchunks), cps, d_seg, nstreams);
    if (d_sym)
        hipLaunchKernelGGL(skip_scatter_kernel<true>, dim3(nchunks), dim3(kSkipBlock), 0, st, d_sym, d_idx, per, cps, skip_rows, bases,
                           d_sym_out, d_idx_out);
    else
        hipLaunchKernelGGL(skip_scatter_kernel<false>, dim3(nchunks), dim3(kSkipBlock), 0, st, d_sym, d_idx, per, cps, skip_rows, bases,
                           d_sym_out, d_idx_out);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}

extern "C" int basic_skip_expand_dev(const int32_t *d_sym_compact, const int32_t *d_idx_dense, int nstreams, int64_t per, int skip_rows,
                                     void *d_scratch, int32_t *d_sym_dense_out, void *hip_stream)
{
    BASIC_REQUIRE(d_sym_compact && d_sym_dense_out && d_sym_dense_out != d_sym_compact && d_sym_dense_out != d_idx_dense,
                  "skip_expand: bad argument (out of place)");
    int cps = 0, nchunks = 0;
    const int rc = skip_plan(d_idx_dense, nstreams, per, skip_rows, d_scratch, &cps, &nchunks);
    if (rc) return rc;
    const hipStream_t st = as_stream(hip_stream);
    int64_t *bases = static_cast<int64_t *>(d_scratch);
    hipLaunchKernelGGL(skip_count_kernel, dim3(nchunks), dim3(kSkipBlock), 0, st, d_idx_dense, per, cps, skip_rows, bases);
    hipLaunchKernelGGL(skip_scan_kernel, dim3(1), dim3(kSkipScanBlock), 0, st, bases, static_cast<int64_t>(nchunks), cps,
                       static_cast<int64_t *>(nullptr), nstreams);
    hipLaunchKernelGGL(skip_expand_kernel, dim3(nchunks), dim3(kSkipBlock), 0, st, d_sym_compact, d_idx_dense, per, cps, skip_rows, bases,
                       d_sym_dense_out);
    BASIC_HIP_TRY(hipGetLastError());
    return BASIC_OK;
}
