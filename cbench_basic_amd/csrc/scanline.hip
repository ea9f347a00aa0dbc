// Persistent scan-line autoregressive coding loop: ONE launch walks all coding steps of a batch -- H*W of them in raster order,
// or, for an encode call under the wavefront schedule of the batched kernel (the rows of an image in parallel, each
// ksize / 2 + 2 columns behind the row above), W + (ksize / 2 + 2) * (H - 1); under its band schedule (the same steps, an image's
// rows sharing W / (ksize / 2 + 2) + 1 columns of a tile) a batch of any size and height, in as many launches as it needs.
//
// Reference: TopoGroupPGMPriorCoder._encode_with_pgm / _pgm_generate (cbench/modules/prior_model/prior_coder/pgm_coder.py:
// 912-981) with the "scanline" topo groups (one group per spatial position, raster order, :1416-1491), the masked 5x5
// context convolution (cbench/nn/layers/masked_conv.py:102-228: for scan-line groups the mask keeps exactly the causal
// raster neighbours) and the 1x1 parameter-merger layers (masked_conv.py:262-300 / pgm_coder.py:1606-1638: dense for one
// channel group), followed by the Gaussian index / quantise step (pgm_coder.py:735-821, 927-941).
//
// Per step the reference (and this library's per-step path) launches ~6-8 tiny dependent kernels; at batch 1 a Kodak-shaped
// latent has 1,536 steps, so the loop is pure launch + dependent-load latency (65-100 us per step).  Here the weights of
// every layer (7.6 MB for C = 192) are spread ONCE over the LDS of `nwg` compute units -- workgroup w owns a fixed slice of
// the output rows of every layer -- and a step is: every workgroup computes its rows of a layer for all images (inputs
// staged in LDS, one wave per dot product), publishes them with write-through (sc1) stores, and all workgroups meet at a
// device-wide barrier before the next layer.  Four barriers per coding step instead of four-plus kernel boundaries with
// their dependent weight re-reads.
//
// Summation order.  The integers coded here must equal, bit for bit, what the per-step path (csrc/mconv.hip) derives from
// the same layers at any batch size -- a stream may be encoded by one path and decoded by the other.  Every dot product is
// therefore evaluated in mconv.hip's CANONICAL order: the K axis of a layer (context layer: [causal tap][channel]; dense
// layer: its input channels in `in_groups` equal groups) is cut, group by group, into blocks of BASIC_MCONV_BLOCK_CHANNELS
// channels; a block's partial is one fp32 FMA chain over its channels in ascending order starting from zero (= the
// v_mfma_f32_32x32x2_f32 chain of the masked convolution, scripts/micro/mfma_arith.hip); the partials are added in block
// order, then the bias.  Taps outside the image enter as zeros, as the masked-out slabs do there.
//
// Cross-workgroup exchange (round 3): DATA-TAGGED GRANULES.  Every value one workgroup hands to the others -- a layer output,
// a coded latent, a (mean, table row) pair for the decoder wavefronts -- travels as ONE naturally aligned 8-byte word
// { float bits | tag << 32 } written with an agent-scope (sc1, write-through) store and read with agent-scope loads; the tag
// is the coding step + 1 for the per-step buffers and the position + 1 for the position-major copy of the coded latent.  A
// consumer polls the word until its tag is the one it expects: the 8-byte store is single-copy atomic, so a matching tag means
// the value beside it is the matching value, and no barrier, no store drain and no separate flag is needed -- a layer
// exchange costs one store-to-load propagation (~2 us) instead of store drain + device barrier + loads (~5 us, measured in
// round 2).  The buffers are zeroed before the launch (tag 0 never matches).  Overwriting is safe without a second
// handshake: workgroup X can write step p+1 of layer l only after it has consumed step p+1 of layer l-1 from EVERY workgroup
// (for l = 0: position p of the coded latent from every producer), and a workgroup that has produced that has -- in program
// order -- already consumed step p of layer l.  Every poll is bounded (kSpinLimit, and the launch's error flag is checked while
// spinning): a launch whose grid is not fully resident gives up and reports it instead of hanging.  One workgroup per compute
// unit (the LDS footprint guarantees it), as MI355X_MICROARCH.md's inter-workgroup visibility section requires of spin-waits.
//
// Host side.  Everything that DECIDES how a call runs -- the constants shared with the kernels, the integer geometry of a plan
// (scan_geometry), the scratch and LDS layouts and the planner (plan_scan) -- is in scan_plan.h, which needs no HIP and is checked on
// the CPU (scan_plan_check.cpp, tests/test_cpu_scan_plan.py).  This file keeps what needs HIP: the kernels, ScanArgs, the plan's
// device state, the scratch allocation, ScanChain, the environment and the device (forced_kernel, make_request), and the launches.
#include "common.h"
#include "scan_plan.h"
#include "wave_decoder.h"

#include <algorithm>
#include <mutex>

#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

using namespace basic;

namespace {

constexpr unsigned kSpinLimit = 4000000u;

struct ScanArgs {
    const float *y;       // [B][C][HW]   (encoder input)
    const float *priorT;  // [B][HW][P]   position-major copy of the prior (nullptr when P == 0)
    float *ybuf;          // [B][C][HW]   coded latent (output)
    uint64_t *yT;         // [B][HW][C]   position-major working copy of the coded latent as granules (tag = position + 1)
    int32_t *sym, *idx;   // [B][HW * C]  position-major: element p * C + c
    const float *table;
    int table_len;
    int B, C, H, W, P;
    int nlayers, ntaps, vec4;   // vec4: every K, row count and C is a multiple of 4 -> 16-byte exchanges and LDS reads
    int rows[kMaxLayers], kdim[kMaxLayers], rpw[kMaxLayers], woff[kMaxLayers], act_after[kMaxLayers];
    int kgroup[kMaxLayers], bpg[kMaxLayers], kpad[kMaxLayers];   // channels / canonical blocks per K group; padded LDS row (see padded_k)
    const float *w[kMaxLayers], *bias[kMaxLayers];
    uint64_t *act[kMaxLayers];   // exchange buffers [B][rows_l] of granules (tag = coding step + 1)
    int tap_off[kMaxTaps], tap_dy[kMaxTaps], tap_dx[kMaxTaps];
    int bc, xs_off, ps_off, tab_off, part_off, part_floats, flag_off, bias_off;   // LDS float offsets (the whole LDS is dynamic)
    int x0_off, early_off, desc_off;   // pipelined kernel only: context window [B][K0], early sums, unit descriptors
    int ncompute;          // workgroups [0, ncompute) compute, the rest decode (4 streams each)
    unsigned *bar;
    int *err;
    long long *prof;   // BASIC_SCAN_PROFILE=1: [layer][4] 100 MHz ticks of workgroup 0 spent staging (incl. waiting) / in the block dots / finishing / in the
                       // Gaussian step, summed over the steps; [4 * kMaxLayers .. +1] = shader clocks and ticks of the whole loop
    // decoder only
    uint64_t *mu;          // [B][C] means of the current step (compute -> decoder workgroups), granules
    uint64_t *idx_step;    // [B][C] table rows of the current step, granules (the row's bits in the value half)
    RansFastView tv;
    const uint32_t *words; // all streams back to back
    const int64_t *word_off;   // [B * lanes + 1]
    int lanes, lane_w;     // lane streams per image (stream b * lanes + k: channels [k * lane_w, (k + 1) * lane_w)); lanes * lane_w == C
    int row_streams;       // 1: the row-stream format -- stream (b * H + r) * lanes + k carries row r of image b (word_off [B * H * lanes + 1])
    // batched kernel only (scanline_batched_kernel; nbt == 0 for the other two): the batch is the fastest dimension of every
    // exchanged array -- yT [HW][C][nbt], act[l] [rows_l][nbt], priorT [HW][P][nbt]; mu / idx_step stay [image][C]
    int nbt;               // columns of the exchange arrays: 32 * column tiles (a column tile = 32 images = the N of an MFMA tile)
    int nw, nd;            // compute workgroups per column tile; the first nd of them hold the dense layers' row tiles
    int bpt;               // canonical blocks per context tap = C / 64
    int nblk[kMaxLayers], rt[kMaxLayers];   // canonical blocks of a layer's K axis; its 32-row tiles
    int ctx_blocks;        // blocks of the first dense layer fed by the context layer (the rest: the prior)
    int tile_off[kMaxLayers];   // dense-role workgroups: LDS float offset of a layer's partial tiles
    float *wlate;          // [compute workgroups][256 threads][32]: a context workgroup's late blocks as A fragments (written by the launch itself)
    // wavefront encode schedule of the batched kernel only (wf_cols == 0 otherwise): a column is (image, row), step t codes column
    // position t - wf_s * row of every row, and the per-position arrays become per-step ones -- yT [steps][C][wf_yw], priorT [steps][P][nbt]
    int wf_cols;           // B * H columns in use
    int wf_s;              // steps a row starts after the row above it: ksize / 2 + 2
    int wf_steps;          // W + wf_s * (H - 1)
    int wf_yw;             // columns of a yT slab: per image ksize / 2 pad columns (the rows above the image: zeros), then its H rows
    // band schedule only, encode and the decode of row streams (band_A == 0 otherwise; the wf_* fields hold as for the wavefront, B = the images of THIS launch): a lane
    // of a column tile is a SLOT of an image -- image (tile * band_ipt + lane / band_A), slot lane % band_A -- that walks rows slot,
    // slot + band_A, ... of its image one after the other (see the band section in front of scanline_batched_kernel)
    int band_A;            // slots per image: W / wf_s + 1, so a slot's period band_A * wf_s exceeds W
    int band_ipt;          // images per column tile: 32 / band_A
};

typedef float f4 __attribute__((ext_vector_type(4)));
__host__ __device__ __forceinline__ int64_t bm_gran(int c, int col, int nbt);   // batched kernel's exchange layout (defined with it)

__device__ __forceinline__ uint64_t ld_gran(const uint64_t *p)
{
    return __hip_atomic_load(const_cast<uint64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_gran(uint64_t *p, uint32_t bits, uint32_t tag)
{
    __hip_atomic_store(p, static_cast<uint64_t>(bits) | (static_cast<uint64_t>(tag) << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_gran(uint64_t *p, float v, uint32_t tag) { st_gran(p, __float_as_uint(v), tag); }

// Workgroup barrier for LDS hand-overs only: waits for this wave's LDS traffic, NOT for its global stores -- __syncthreads()
// also drains vmcnt, i.e. it would wait ~1-1.5 us per layer for the write-through stores of the granules just published.
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// polls a granule until it carries `tag`; false when the launch is poisoned (bounded spin / another workgroup gave up)
__device__ __forceinline__ bool wait_gran(const ScanArgs &a, const uint64_t *p, uint32_t tag, uint64_t &g)
{
    unsigned spins = 0;
    while (static_cast<uint32_t>(g >> 32) != tag) {
        if (++spins > kSpinLimit || (spins % 1024u == 0u && __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
            __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
        g = ld_gran(p);
    }
    return true;
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// argmin_j |s - table[j]|, first minimum (pgm_coder.py:802-821; same as entropy.hip::nearest_scale).  On a strictly
// increasing table (the scale table is: checked once per workgroup) the minimum lies at the first entry >= s or the one
// before it, the earlier of the two on a tie: a 6-step search instead of a 64-step scan on the step's critical path.
__device__ __forceinline__ int nearest_scale(float s, const float *tab, int n, bool sorted)
{
    if (sorted && __builtin_isfinite(s)) {   // (NaN / infinite scales: the scan below defines the result)
        int lo = 0, hi = n;   // first index with tab[idx] >= s, in [0, n]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (tab[mid] < s) lo = mid + 1; else hi = mid;
        }
        if (lo == 0) return 0;
        if (lo == n) return n - 1;
        return fabsf(s - tab[lo]) < fabsf(s - tab[lo - 1]) ? lo : lo - 1;
    }
    int best = 0;
    float bd = fabsf(s - tab[0]);
    for (int j = 1; j < n; ++j) {
        const float d = fabsf(s - tab[j]);
        if (d < bd) { bd = d; best = j; }
    }
    return best;
}

// ---- inputs of `nb` images for layer l at position p -> xs[bi][k]; every exchanged value is polled until it carries the
//      expected tag (context layer: the neighbour's position + 1; dense layers: this step + 1).  Returns false when poisoned.
__device__ __forceinline__ bool stage_inputs(const ScanArgs &a, int l, int p, int py, int px, int b0, int nb, float *xs)
{
    const int tid = threadIdx.x, HW = a.H * a.W, K = a.kdim[l];
    const int total = nb * K, prev = l ? a.rows[l - 1] : 0;
    constexpr int U = 12;   // loads in flight per thread: the context layer at batch 1 is 9 granules per thread -- ONE round trip, not two
    bool ok = true;
    for (int e0 = tid; e0 < total; e0 += kThreads * U) {
        const uint64_t *src[U];
        uint64_t g[U];
        uint32_t want[U];
        float plain[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {   // all loads of the batch in flight before the first tag is looked at
            const int e = e0 + u * kThreads;
            src[u] = nullptr; g[u] = 0ull; want[u] = 0u; plain[u] = 0.f;
            if (e < total) {
                const int bi = e / K, kk = e - bi * K;
                const int64_t b = b0 + bi;
                if (l == 0) {   // causal neighbourhood of the coded latent: [tap][c]
                    const int t = kk / a.C, c = kk - t * a.C;
                    const int ny = py + a.tap_dy[t], nx = px + a.tap_dx[t];
                    if (ny >= 0 && nx >= 0 && nx < a.W) {
                        src[u] = a.yT + ((b * HW + p + a.tap_off[t]) * a.C + c);
                        want[u] = static_cast<uint32_t>(p + a.tap_off[t] + 1);
                    }
                } else if (kk < prev) {
                    src[u] = a.act[l - 1] + b * prev + kk;
                    want[u] = static_cast<uint32_t>(p + 1);
                } else if (a.priorT) {   // cat(ctx, prior); the prior is an input of the launch: ordinary loads
                    plain[u] = a.priorT[(b * HW + p) * a.P + (kk - prev)];
                }
                if (src[u]) g[u] = ld_gran(src[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * kThreads;
            if (e < total) {
                if (src[u]) {
                    ok = wait_gran(a, src[u], want[u], g[u]) && ok;
                    xs[e] = __uint_as_float(static_cast<uint32_t>(g[u]));
                } else {
                    xs[e] = plain[u];
                }
            }
        }
    }
    // A position at the start of a row has no left neighbour, so nothing above makes it wait for the previous position --
    // but the overwrite argument of the exchange buffers (header comment) needs every workgroup's step p+1 to start after
    // position p is coded: wait for its granules without using the values.
    if (l == 0 && p > 0 && px == 0) {
        for (int e = tid; e < nb * a.C; e += kThreads) {
            const int bi = e / a.C, c = e - bi * a.C;
            const uint64_t *src = a.yT + ((static_cast<int64_t>(b0 + bi) * HW + p - 1) * a.C + c);
            uint64_t g = ld_gran(src);
            ok = wait_gran(a, src, static_cast<uint32_t>(p), g) && ok;
        }
    }
    return ok;
}

// LDS position of element k of a weight row whose K axis has groups of kg channels (bpg blocks each)
__host__ __device__ __forceinline__ int padded_k(int k, int kg, int bpg)
{
    const int g = k / kg, kk = k - g * kg;
    return g * (kg + kBlockPad * bpg) + kk + kBlockPad * (kk / kKB);
}

// ---- one canonical block of one output: an FMA chain over `len` channels in ascending order, starting from zero.  A THREAD
//      owns a (block, image, row) unit; threads of a wave take consecutive rows of the same block (weight rows are padded
//      so that they start on different banks; lanes of one image read the same input address: LDS broadcast).
__device__ __forceinline__ float block_dot(const float *wr, const float *xr, int len, int vec4)
{
    float p = 0.f;
    if (vec4) {
        const f4 *x4 = reinterpret_cast<const f4 *>(xr), *w4 = reinterpret_cast<const f4 *>(wr);
        const int n4 = len >> 2;
        int k4 = 0;
        for (; k4 + 4 <= n4; k4 += 4) {   // 16 channels of loads in flight, one chain
            const f4 x0 = x4[k4], x1 = x4[k4 + 1], x2 = x4[k4 + 2], x3 = x4[k4 + 3];
            const f4 w0 = w4[k4], w1 = w4[k4 + 1], w2 = w4[k4 + 2], w3 = w4[k4 + 3];
#define BASIC_FMA4(WV, XV) p = fmaf(WV[0], XV[0], p); p = fmaf(WV[1], XV[1], p); p = fmaf(WV[2], XV[2], p); p = fmaf(WV[3], XV[3], p)
            BASIC_FMA4(w0, x0); BASIC_FMA4(w1, x1); BASIC_FMA4(w2, x2); BASIC_FMA4(w3, x3);
        }
        for (; k4 < n4; ++k4) { const f4 xv = x4[k4], wv = w4[k4]; BASIC_FMA4(wv, xv); }
#undef BASIC_FMA4
    } else {
        for (int k = 0; k < len; ++k) p = fmaf(wr[k], xr[k], p);
    }
    return p;
}

// ---- in-place rANS decoder of ONE stream held by one wavefront (decode_stream semantics, csrc/ans/rans64.cpp:501-598;
//      the search image, the arithmetic and the chunk schedule of rans_decode_fast_kernel in rans.hip: a lone wave is bound by
//      its instruction count, so a symbol's 16-byte image entry -- which depends on its table row only, not on the coder
//      state -- is read from LDS two symbols ahead, every lane advances the state for ITS candidate symbol, and one
//      compare + ballot picks the lane that is right; renormalisation, the bypass sentinel and wide rows (image frequency 0)
//      all hide behind the single test "new state < 2^31")
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

using wavedec::static_pairs;
using wavedec::WaveDecoder;   // the serial rANS chain of one stream (wave_decoder.h)

// ================= decoder workgroups: one wavefront per stream, the search image in LDS =================
// An image is one stream, or -- the lane-stream format, a.lanes > 1 -- a.lanes of them: stream b * lanes + k carries the symbols of
// channels [k * lane_w, (k + 1) * lane_w) in coding order, so the waves of an image's lanes decode a position side by side, each
// fetching its own channels' (row, mean) granules and publishing at its own channels.  lane_w is a multiple of 16: the batched
// exchange layout stays linear in a chunk's first channel (multiples of 4), and a chunk's stores stay whole 64-byte runs.
// LANES = false is the one-stream loop with its bounds as they always were (stream = image, channels [0, C)): a call without
// lanes runs the code it ran before the format existed.
//
// ROWS: the row-stream format (a.row_streams): stream (b * H + r) * lanes + k carries row r only.  (ROWS = 1 is instantiated for LANES
// false and true like the loop without rows -- with run-time lanes it left the pipelined kernel 20 bytes of private segment --,
// ROWS = 2 takes its lanes at run time, 1 included.)
//   * ROWS = 1, the raster kernels: a wave still serves (image, lane) and walks all H * W steps, but at every row start it
//     re-initialises its WaveDecoder on the row's stream: its word offsets and the head's three 64-word blocks are loaded there,
//     two dependent round trips per row on the step's path (kept there on purpose: see DESIGN.md section 3).
//   * ROWS = 2, the wavefront decode launch (scanline_batched_kernel<true, true>): one wave per (column, lane) = per stream.  Row r
//     starts in step wf_s * r; until then the wave sleeps between polls of its first granule (a wave polling at full rate for up to
//     wf_s * (H - 1) steps would take issue slots and memory requests from the decoder waves at work beside it), bounded like
//     every spin.  Then W times "wait for the column's (row, mean) granules with the step's tag -> decode_chunk -> publish" into
//     slab wf_s * r + c at the row's true column, and into sym / idx / ybuf at position r * W + c; then it returns.  The zeros of
//     the steps in which the column is idle are published by the compute workgroups, never from here (they pace the tile's
//     context workgroups: see the band section in front of scanline_batched_kernel).
//   * ROWS = 3, the band decode launch (scanline_batched_kernel<true, true, true>): one wave per (image, slot, lane), NOT per row --
//     an image brings min(band_A, H) * lanes of them whatever its height, which is what lets a launch hold many and tall images.
//     Slot j's wave decodes rows j, j + band_A, ... one after the other, each exactly as a ROWS = 2 wave decodes its only row: the
//     sleeping wait for the tag of the row's first step wf_s * r on the slot's MFMA column of mu / idx_step (tile * 32 + image in
//     tile * band_A + slot: where the slot's compute lane publishes), W steps of wait -> decode_chunk -> publish into slab
//     wf_s * r + c at the row's true column and into sym / idx / ybuf at r * W + c.  Between two rows the slot idles
//     band_A * wf_s - W steps (1 .. wf_s: its compute lane publishes zeros); the wave re-initialises its WaveDecoder on the next
//     row's stream there (restart: the two dependent round trips that sit on the step's path in the raster kernels), before it
//     goes to sleep on the next row's first tag -- which the slot's column cannot carry earlier: its previous tag is the last
//     step of the row just decoded.
template <bool LANES, int ROWS = 0>
__device__ __forceinline__ void decoder_loop(const ScanArgs &a, float *lds)
{
    static_assert(ROWS < 2 || LANES, "the wavefront's and the band's row streams take their lanes at run time");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wg = blockIdx.x;
    const int HW = a.H * a.W;
    uint32_t *img = reinterpret_cast<uint32_t *>(lds);
    for (int e = tid; e < a.tv.image_words; e += kThreads) img[e] = a.tv.image[e];
    // per table row {image offset, size, symbol offset}: three dependent global loads per chunk on the step's critical path otherwise
    u32x4 *rowtab = reinterpret_cast<u32x4 *>(img + ((a.tv.image_words + 3) & ~3));
    for (int r = tid; r < a.tv.rows; r += kThreads)
        rowtab[r] = u32x4{a.tv.meta[r], static_cast<uint32_t>(a.tv.sizes[r]), static_cast<uint32_t>(a.tv.offsets[r]), 0u};
    __syncthreads();
    const int s = (wg - a.ncompute) * (kThreads / 64) + wave;
    const int bslots = ROWS == 3 ? (a.band_A < a.H ? a.band_A : a.H) : 1;   // ROWS = 3: the slots of an image that have a row
    if (s >= (ROWS == 3 ? a.B * bslots * a.lanes : ROWS == 2 ? a.wf_cols * a.lanes : LANES ? a.B * a.lanes : a.B)) return;
    const int q = LANES ? s / a.lanes : s;             // the column of mu / idx_step: the image, or (ROWS = 2) image * H + row; ROWS = 3: image * bslots + slot
    const int b = ROWS == 3 ? q / bslots : ROWS == 2 ? q / a.H : q;
    int wr = ROWS == 3 ? q - b * bslots : ROWS == 2 ? q - b * a.H : 0;   // ROWS = 2: this stream's row (ROWS = 3: the slot = its first row),
    int t0 = ROWS >= 2 ? a.wf_s * wr : 0;              // the step it starts in
    const int kl = LANES ? s - q * a.lanes : 0;
    const int cbeg = LANES ? kl * a.lane_w : 0, cend = LANES ? cbeg + a.lane_w : a.C;   // this stream's channels
    // (ROWS = 3: the slot's MFMA column -- its image's tile, the image inside the tile, the slot)
    const int mcol = ROWS == 3 ? (b / a.band_ipt) * 32 + (b % a.band_ipt) * a.band_A + wr : q;
    const uint64_t *pi0 = a.idx_step + static_cast<int64_t>(mcol) * a.C, *pm0 = a.mu + static_cast<int64_t>(mcol) * a.C;
    // a serial chain: never lose the issue arbitration to the waves spinning beside it (a wavefront row: once it has started)
    if constexpr (ROWS < 2) __builtin_amdgcn_s_setprio(3);
    WaveDecoder d;
    const int nl = LANES ? a.lanes : 1;
    int sr = ROWS == 3 ? (b * a.H + wr) * nl + kl : ROWS == 1 ? b * a.H * nl + kl : s, left = a.W;   // ROWS = 1 (3): the current row's stream, the positions left in that row
    {
        const int64_t w0 = a.word_off[sr];
        d.init(img, a.words + w0, static_cast<int>(a.word_off[sr + 1] - w0), a.tv.precision, a.tv.bypass_precision, a.tv.bypass != 0, -1, 0ull, lane);
    }
    if constexpr (ROWS == 2) {
        if (t0 > 0) {   // a row that starts late: one granule, polled between sleeps (wave-uniform: every lane reads the same word)
            unsigned spins = 0;
            while (static_cast<uint32_t>(ld_gran(pi0 + cbeg) >> 32) != static_cast<uint32_t>(t0 + 1)) {
                if (++spins > kSpinLimit || (spins % 64u == 0u && __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                    __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    return;
                }
                __builtin_amdgcn_s_sleep(32);   // 32 x 64 clocks: about a microsecond, a twentieth of a step
            }
        }
        __builtin_amdgcn_s_setprio(3);
    }
    // ROWS = 3: the same wait, before every row of the slot (kept apart from the block above, which stays as it was: the wavefront
    // launch runs the code it ran before the band existed); false = poisoned launch
    auto band_row_start = [&]() -> bool {
        unsigned spins = 0;
        while (static_cast<uint32_t>(ld_gran(pi0 + cbeg) >> 32) != static_cast<uint32_t>(t0 + 1)) {
            if (++spins > kSpinLimit || (spins % 64u == 0u && __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return false;
            }
            __builtin_amdgcn_s_sleep(32);
        }
        return true;
    };
    if constexpr (ROWS == 3) {
        if (t0 > 0 && !band_row_start()) return;
        __builtin_amdgcn_s_setprio(3);
    }
    // where a chunk's results go: a uniform pointer per (step, chunk) + a lane term that never changes (channel c0 + lane; the
    // batched exchange layout is linear in c0: bm_gran(c0 + l) = bm_gran(l) + c0 * nbt for chunk starts c0)
    const int64_t bC = static_cast<int64_t>(b) * a.C;
    const int YW = ROWS >= 2 ? a.wf_yw : a.nbt;        // columns of a slab of the coded latent (wavefront, band: with the pad columns)
    int ycol = ROWS >= 2 ? b * (a.H + a.wf_s - 2) + a.wf_s - 2 + wr : b;
    uint32_t lane_g = YW ? static_cast<uint32_t>(bm_gran(lane, ycol, YW)) : static_cast<uint32_t>(lane);
    const uint32_t lane_y = static_cast<uint32_t>(lane) * static_cast<uint32_t>(HW);
    // ROWS = 3: the slot's rows wr, wr + band_A, ... below H, W positions each; i0 = the loop index at which the current row started
    const int band_count = ROWS == 3 ? ((a.H - wr + a.band_A - 1) / a.band_A) * a.W : 0;
    int i0 = 0;
    for (int i = 0; i < (ROWS == 3 ? band_count : ROWS == 2 ? a.W : HW); ++i) {
        if constexpr (ROWS == 3) {
            if (left == 0) {   // the slot's next row: its stream, its first step, its column of the slabs -- in the slot's idle steps,
                sr += a.band_A * nl; left = a.W;   // where nothing waits for this wave
                const int64_t w0 = a.word_off[sr];
                d.restart(a.words + w0, static_cast<int>(a.word_off[sr + 1] - w0), lane);
                wr += a.band_A; t0 = a.wf_s * wr; i0 = i;
                ycol += a.band_A;
                lane_g = static_cast<uint32_t>(bm_gran(lane, ycol, YW));
                if (!band_row_start()) return;
            }
            --left;
        }
        const int p = ROWS == 3 ? wr * a.W + i - i0 : ROWS == 2 ? wr * a.W + i : i;   // the position inside the image,
        const int sl = ROWS == 3 ? t0 + i - i0 : ROWS == 2 ? t0 + i : i;              // the step: its tag, and its slab of the coded latent
        const uint32_t tag = static_cast<uint32_t>(sl + 1);
        if constexpr (ROWS == 1) {
            if (left == 0) {   // a row start: the row's stream
                sr += nl; left = a.W;
                const int64_t w0 = a.word_off[sr];
                d.restart(a.words + w0, static_cast<int>(a.word_off[sr + 1] - w0), lane);
            }
            --left;
        }
        // this step's (table row, mean) granules come from the compute workgroups that own the channels; the next chunk's
        // are requested before the current chunk is decoded
        uint64_t gi = 0ull, gm = 0ull;
        if (cbeg + lane < cend) { gi = ld_gran(pi0 + cbeg + lane); gm = ld_gran(pm0 + cbeg + lane); }
        for (int c0 = cbeg; c0 < cend; c0 += 64) {
            const int c = c0 + lane;
            bool ok = true;
            d.line_up(lane);   // the chunk's 64 stream words, cut while the step's parameters are still on their way
            const long long tw0 = a.prof ? wall_clock64() : 0;
            if (c < cend) ok = wait_gran(a, pi0 + c, tag, gi) && wait_gran(a, pm0 + c, tag, gm);
            if (__ballot(!ok) != 0ull) return;   // poisoned launch: wave-uniform exit
            const long long tw1 = a.prof ? wall_clock64() : 0;
            int32_t row = static_cast<int32_t>(static_cast<uint32_t>(gi));
            const float mu = __uint_as_float(static_cast<uint32_t>(gm));
            gi = 0ull; gm = 0ull;
            if (c + 64 < cend) { gi = ld_gran(pi0 + c + 64); gm = ld_gran(pm0 + c + 64); }
            row = row < 0 ? 0 : (row >= a.tv.rows ? a.tv.rows - 1 : row);
            const u32x4 rt = rowtab[row];
            const int cnt = (cend - c0) < 64 ? (cend - c0) : 64;
            const long long tc2 = a.prof ? clock64() : 0;
            const int32_t mine = d.decode_chunk(rt[0], static_cast<int32_t>(rt[1]), cnt, lane) - 1;
            const long long tc3 = a.prof ? clock64() : 0;
            if (c < cend) {
                const int32_t value = mine + static_cast<int32_t>(rt[2]);
                const float v = static_cast<float>(value) + mu;           // pgm_coder.py:973-978
                const int64_t at = bC * HW + static_cast<int64_t>(p) * a.C + c0;   // [b][p][c0] of sym / idx
                uint64_t *yt = a.yT + (YW ? (static_cast<int64_t>(sl) * a.C + c0) * YW : (static_cast<int64_t>(b) * HW + p) * a.C + c0);
                st_gran(yt + lane_g, v, tag);   // first: the compute workgroups wait for it
                (a.sym + at)[lane] = value;
                (a.idx + at)[lane] = row;
                (a.ybuf + ((bC + c0) * HW + p))[lane_y] = v;
            }
            if (a.prof) {   // first stream: ticks waiting for the step's parameters / decoding and publishing
                const long long tc4 = clock64(), tw4 = wall_clock64();   // (read before the slots are touched: their updates wait for memory)
                if (s == 0 && lane == 0) {
                    a.prof[4 * kMaxLayers + 2] += tw1 - tw0;
                    a.prof[4 * kMaxLayers + 3] += tw4 - tw1;
                    a.prof[4 * kMaxLayers + 4] += tc3 - tc2;            // shader clocks inside decode_chunk
                    a.prof[4 * kMaxLayers + 5] += tc4 - tc3;            // ... publishing
                    a.prof[4 * kMaxLayers + 6] = d.position();
                }
            }
        }
    }
}

// WF: the decoder workgroups of the wavefront decode launch (row streams only: nothing else has one); BAND: of the band decode launch
template <bool WF = false, bool BAND = false>
__device__ __forceinline__ void decoder_workgroup(const ScanArgs &a, float *lds)
{
    if constexpr (BAND) decoder_loop<true, 3>(a, lds);
    else if constexpr (WF) decoder_loop<true, 2>(a, lds);
    else if (a.row_streams) { if (a.lanes > 1) decoder_loop<true, 1>(a, lds); else decoder_loop<false, 1>(a, lds); }
    else if (a.lanes > 1) decoder_loop<true>(a, lds);
    else decoder_loop<false>(a, lds);
}

template <bool DECODE>
__global__ __launch_bounds__(kThreads) void scanline_persistent_kernel(const ScanArgs a)
{
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int wg = blockIdx.x;
    const int HW = a.H * a.W;
    const int last = a.nlayers - 1;

    if (DECODE && wg >= a.ncompute) { decoder_workgroup(a, lds); return; }

    // ================= compute workgroups: a fixed slice of every layer's rows, weights resident in LDS =================
    int rows_w[kMaxLayers];
    for (int l = 0; l < a.nlayers; ++l) {
        int r = a.rows[l] - wg * a.rpw[l];
        r = r < 0 ? 0 : (r > a.rpw[l] ? a.rpw[l] : r);
        rows_w[l] = r;
        const float *src = a.w[l] + static_cast<int64_t>(wg) * a.rpw[l] * a.kdim[l];
        float *dst = lds + a.woff[l];
        const int Kl = a.kdim[l], Kp = a.kpad[l];
        for (int e = tid; e < r * Kl; e += kThreads) { const int rr = e / Kl; dst[rr * Kp + padded_k(e - rr * Kl, a.kgroup[l], a.bpg[l])] = src[e]; }
    }
    float *tab = lds + a.tab_off;
    for (int e = tid; e < a.table_len; e += kThreads) tab[e] = a.table[e];
    float *xs = lds + a.xs_off, *ps = lds + a.ps_off, *part = lds + a.part_off;
    int *s_flag = reinterpret_cast<int *>(lds + a.flag_off);
    // this workgroup's biases in LDS (a global load per output on the finishing threads cost ~1 us per layer and step)
    float *bias_l[kMaxLayers];
    {
        int off = a.bias_off;
        for (int l = 0; l < a.nlayers; ++l) {
            bias_l[l] = lds + off;
            for (int e = tid; e < rows_w[l]; e += kThreads) bias_l[l][e] = a.bias[l] ? a.bias[l][wg * a.rpw[l] + e] : 0.f;
            off += a.rpw[l];
        }
    }
    if (tid == 0) { s_flag[0] = 0; s_flag[1] = 1; }
    __syncthreads();
    for (int e = tid; e + 1 < a.table_len; e += kThreads)
        if (!(tab[e] < tab[e + 1])) s_flag[1] = 0;   // not strictly increasing: nearest_scale scans
    __syncthreads();
    const bool tab_sorted = s_flag[1] != 0;
    const long long loop_c0 = a.prof ? clock64() : 0, loop_t0 = a.prof ? wall_clock64() : 0;
    for (int p = 0; p < HW; ++p) {
        const int py = p / a.W, px = p - py * a.W;
        const uint32_t tag = static_cast<uint32_t>(p + 1);
        for (int l = 0; l <= last; ++l) {
            const int K = a.kdim[l], rw = rows_w[l];
            if (rw == 0) continue;   // a workgroup without rows of this layer has nothing to produce -- and nothing to wait for
            const float *wl = lds + a.woff[l];
            const int r_first = wg * a.rpw[l];
            for (int b0 = 0; b0 < a.B; b0 += a.bc) {
                const int nb = (a.B - b0) < a.bc ? (a.B - b0) : a.bc;
                const long long t0 = a.prof ? wall_clock64() : 0;
                // encoder: this thread's latent of the Gaussian step, requested before the last layer's inputs are waited for
                float y_pre = 0.f;
                if (!DECODE && l == last && tid < nb * (rw >> 1)) {
                    const int bi = tid / (rw >> 1), j = tid - bi * (rw >> 1);
                    y_pre = a.y[((static_cast<int64_t>(b0 + bi)) * a.C + (r_first >> 1) + j) * HW + p];
                }
                const bool ok = stage_inputs(a, l, p, py, px, b0, nb, xs);
                if (!ok) *s_flag = 1;    // (a flag in the dynamic LDS: __syncthreads_or would add static LDS on top of the 160 KB)
                __syncthreads();
                if (*s_flag) return;     // poisoned launch: the whole workgroup leaves
                const long long t1 = a.prof ? wall_clock64() : 0;
                long long t2 = t1, t3 = t1;
                // units = (canonical block, image, row), one FMA chain each; `part` holds one round of partials as
                // [block][item]; the finishing threads add an item's partials in block order, then bias and activation
                const int items = nb * rw, Kp = a.kpad[l];
                const int kg = a.kgroup[l], bpg = a.bpg[l], nblk = (K / kg) * bpg;
                const int per_round = items < a.part_floats / nblk ? items : a.part_floats / nblk;
                for (int i0 = 0; i0 < items; i0 += per_round) {
                    const int n_it = (items - i0) < per_round ? (items - i0) : per_round;
                    for (int u = tid; u < n_it * nblk; u += kThreads) {
                        const int blk = u / n_it, it = u - blk * n_it, item = i0 + it;
                        const int bi = item / rw, r = item - bi * rw;
                        const int g = blk / bpg, j = blk - g * bpg;
                        const int k0 = g * kg + j * kKB, len = (kg - j * kKB) < kKB ? (kg - j * kKB) : kKB;
                        part[u] = block_dot(wl + r * Kp + g * (kg + kBlockPad * bpg) + j * (kKB + kBlockPad), xs + bi * K + k0, len, a.vec4);
                    }
                    lds_barrier();
                    if (a.prof && wg == 0 && tid == 0) t2 = wall_clock64();
                    for (int it = tid; it < n_it; it += kThreads) {
                        const int item = i0 + it, bi = item / rw, r = item - bi * rw;
                        float v = 0.f;
                        for (int blk = 0; blk < nblk; ++blk) v += part[blk * n_it + it];
                        v += bias_l[l][r];
                        if (a.act_after[l]) v = v > 0.f ? v : 0.01f * v;   // LeakyReLU(0.01)
                        if (l < last) st_gran(a.act[l] + static_cast<int64_t>(b0 + bi) * a.rows[l] + r_first + r, v, tag);
                        else ps[bi * a.rpw[l] + r] = v;
                    }
                    lds_barrier();   // `part` is reused by the next round; ps is complete for the Gaussian step
                    if (a.prof && wg == 0 && tid == 0) t3 = wall_clock64();
                }
                if (l == last) {
                    // ---- Gaussian step on this workgroup's (mean, scale) pairs: rows 2c, 2c + 1 ("split_interleave")
                    const int pairs = rw >> 1, c_first = r_first >> 1;
                    for (int it = tid; it < nb * pairs; it += kThreads) {
                        const int bi = it / pairs, j = it - bi * pairs;
                        const int64_t b = b0 + bi;
                        const int c = c_first + j;
                        const float mu = ps[bi * a.rpw[l] + 2 * j], sg = ps[bi * a.rpw[l] + 2 * j + 1];
                        const int row = nearest_scale(sg, tab, a.table_len, tab_sorted);
                        if (DECODE) {
                            st_gran(a.idx_step + b * a.C + c, static_cast<uint32_t>(row), tag);
                            st_gran(a.mu + b * a.C + c, mu, tag);
                        } else {
                            const int64_t e = (b * a.C + c) * HW + p;
                            const int64_t o = b * a.C * HW + static_cast<int64_t>(p) * a.C + c;
                            const float q = rintf((it == tid ? y_pre : a.y[e]) - mu);          // torch.round: half to even
                            st_gran(a.yT + (b * HW + p) * a.C + c, q + mu, tag);   // first: every workgroup's next step waits for it
                            a.idx[o] = row;
                            a.sym[o] = static_cast<int32_t>(q);
                            a.ybuf[e] = q + mu;
                        }
                    }
                }
                lds_barrier();   // xs / ps are reused by the next chunk
                if (a.prof && wg == 0 && tid == 0) {
                    a.prof[4 * l] += t1 - t0;
                    a.prof[4 * l + 1] += t2 - t1;
                    a.prof[4 * l + 2] += t3 - t2;
                    a.prof[4 * l + 3] += wall_clock64() - t3;
                }
            }
        }
    }
    if (a.prof && wg == 0 && tid == 0) {
        a.prof[4 * kMaxLayers] = clock64() - loop_c0;
        a.prof[4 * kMaxLayers + 1] = wall_clock64() - loop_t0;
    }
}

// ================================================================================================================
// Pipelined variant for the batches whose whole working set fits the LDS beside the weights (batch 1-2 of the BaSIC
// coder: the reference harness's setting).  Same exchange protocol, same canonical sums, same results; what changes is
// the length of the dependent chain of a coding step:
//   * context layer split in two.  Of the ntaps causal taps only the LAST -- the left neighbour, position p - 1 -- is
//     coded during the previous step; the other taps' blocks (the first (ntaps - 1) * blocks-per-tap of the canonical
//     order) are summed one step AHEAD, right after this workgroup has published its context rows and while the next
//     layer's inputs are still in flight.  On the critical path stay C granules, blocks-per-tap dot products per row
//     and a short sum, instead of ntaps * C granules and the whole layer.  (Needs a latent at least ksize / 2 + 2 columns
//     wide: in a narrower one the tap up and to the right of position p + 1 IS position p or later; the host then takes the
//     generic kernel);
//   * a (block, image, row) unit's addresses are computed once per launch (descriptor table in LDS), not with four
//     integer divisions per unit and step -- a workgroup is four lone waves, each issuing one instruction per ~8-10
//     clocks, so instruction count IS the latency;
//   * a unit loads its whole block (16 + 16 16-byte LDS reads) before the FMA chain starts;
//   * the last layer's finishing thread owns a (mean, scale) pair and runs the Gaussian step itself: no hand-over
//     through LDS, two workgroup barriers per layer instead of three.
// ================================================================================================================

// all `len` channels of a block in flight, then the chain (len == kKB, vec4); the generic block_dot otherwise
__device__ __forceinline__ float block_dot_preloaded(const float *wr, const float *xr, int len, int vec4)
{
    if (len == kKB && vec4) {
        const f4 *x4 = reinterpret_cast<const f4 *>(xr), *w4 = reinterpret_cast<const f4 *>(wr);
        f4 xv[kKB / 4], wv[kKB / 4];
#pragma unroll
        for (int i = 0; i < kKB / 4; ++i) { wv[i] = w4[i]; xv[i] = x4[i]; }
        float p = 0.f;
#pragma unroll
        for (int i = 0; i < kKB / 4; ++i) {
            p = fmaf(wv[i][0], xv[i][0], p); p = fmaf(wv[i][1], xv[i][1], p); p = fmaf(wv[i][2], xv[i][2], p); p = fmaf(wv[i][3], xv[i][3], p);
        }
        return p;
    }
    return block_dot(wr, xr, len, vec4);
}

// v + part[0] + part[stride] + ... (n terms, in that order); eight LDS reads in flight per round -- a finishing thread is
// alone on its SIMD, a read-wait-add loop costs ~130 clocks per term
__device__ __forceinline__ float sum_partials(float v, const float *part, int stride, int n)
{
    int blk = 0;
    for (; blk + 8 <= n; blk += 8) {
        float t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = part[(blk + i) * stride];
#pragma unroll
        for (int i = 0; i < 8; ++i) v += t[i];
    }
    for (; blk + 2 <= n; blk += 2) {
        const float t0 = part[blk * stride], t1 = part[(blk + 1) * stride];
        v += t0; v += t1;
    }
    if (blk < n) v += part[blk * stride];
    return v;
}

// Two neighbouring granules with one 16-byte load.  Each 8-byte half validates itself by its own tag, so nothing is asked
// of the load beyond what an aligned 8-byte access gives; volatile = cache-bypassing (sc0 sc1) on gfx950, as ld_gran's.
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u64x2 ld_gran2(const uint64_t *p)
{
    typedef const volatile u64x2 __attribute__((address_space(1))) *global_ptr;   // (a generic pointer would make it a flat load)
    return *(global_ptr)(reinterpret_cast<uintptr_t>(p));
}
__device__ __forceinline__ bool tags_are(const u64x2 &g, uint32_t want)
{
    return static_cast<uint32_t>(g[0] >> 32) == want && static_cast<uint32_t>(g[1] >> 32) == want;
}
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 values_of(const u64x2 &g)
{
    return f2{__uint_as_float(static_cast<uint32_t>(g[0])), __uint_as_float(static_cast<uint32_t>(g[1]))};
}

// n granule pairs src[2i], src[2i + 1] (all carrying `want` once written) -> dst[2i], dst[2i + 1]; thread i, i + 256, ...,
// two pairs of a thread in flight.  No divisions, no per-element address arithmetic beyond one add: the workgroup's
// waves are alone on their SIMDs and issue one instruction per ~10 clocks.
__device__ __forceinline__ bool stage_pairs(const ScanArgs &a, const uint64_t *src, int n, uint32_t want, float *dst)
{
    bool ok = true;
    for (int i0 = threadIdx.x; i0 < n; i0 += 2 * kThreads) {
        const int i1 = i0 + kThreads;
        const bool two = i1 < n;
        u64x2 g0 = ld_gran2(src + 2 * i0), g1 = two ? ld_gran2(src + 2 * i1) : u64x2{0ull, 0ull};
        unsigned spins = 0;
        for (;;) {
            const bool r0 = !tags_are(g0, want), r1 = two && !tags_are(g1, want);
            if (!r0 && !r1) break;
            if (++spins > kSpinLimit || (spins % 1024u == 0u && __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = false;
                break;
            }
            if (r0) g0 = ld_gran2(src + 2 * i0);
            if (r1) g1 = ld_gran2(src + 2 * i1);
        }
        *reinterpret_cast<f2 *>(dst + 2 * i0) = values_of(g0);
        if (two) *reinterpret_cast<f2 *>(dst + 2 * i1) = values_of(g1);
    }
    return ok;
}

// per-thread state of one layer of the pipelined kernel; the layer index is a compile-time constant wherever these are
// used, so they live in registers
struct LayerRegs {
    int rw, n_it, K, prev, nblk, units, dbase, r_first;
    float bias0, bias1;   // of this thread's finishing item (last layer: of its (mean, scale) pair)
    int fin_bi, fin_r;    // this thread's finishing item: image, row (last layer: pair)
};

template <bool DECODE>
__global__ __launch_bounds__(kThreads) void scanline_pipelined_kernel(const ScanArgs a)
{
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wg = blockIdx.x;
    const int HW = a.H * a.W, B = a.B, C = a.C;
    const int last = a.nlayers - 1;
    if (DECODE && wg >= a.ncompute) { decoder_workgroup(a, lds); return; }

    // ---- this workgroup's weight slices, scale table, unit descriptors
    float *tab = lds + a.tab_off;
    for (int e = tid; e < a.table_len; e += kThreads) tab[e] = a.table[e];
    float *x0 = lds + a.x0_off, *xs = lds + a.xs_off, *part = lds + a.part_off, *early = lds + a.early_off;
    float *part_e = lds + a.early_off + ((B * a.rpw[0] + 3) & ~3);   // the early blocks' partials: not shared with the dense layers
    uint2 *desc = reinterpret_cast<uint2 *>(lds + a.desc_off);
    int *s_flag = reinterpret_cast<int *>(lds + a.flag_off);
    LayerRegs L[kMaxLayers];
    int pairs = 0, my_c = 0, my_b = 0;   // the last layer's (mean, scale) pairs of this workgroup; this thread's channel and image
    {
        int db = 0;
#pragma unroll
        for (int l = 0; l < kMaxLayers; ++l) {
            L[l] = LayerRegs{};
            if (l >= a.nlayers) continue;
            int r = a.rows[l] - wg * a.rpw[l];
            r = r < 0 ? 0 : (r > a.rpw[l] ? a.rpw[l] : r);
            const int Kl = a.kdim[l], Kp = a.kpad[l], kg = a.kgroup[l], bpg = a.bpg[l];
            {
                const float *src = a.w[l] + static_cast<int64_t>(wg) * a.rpw[l] * Kl;
                float *dst = lds + a.woff[l];
                for (int e = tid; e < r * Kl; e += kThreads) { const int rr = e / Kl; dst[rr * Kp + padded_k(e - rr * Kl, kg, bpg)] = src[e]; }
            }
            L[l].rw = r; L[l].n_it = B * r; L[l].K = Kl; L[l].prev = l ? a.rows[l - 1] : 0;
            L[l].nblk = (Kl / kg) * bpg; L[l].units = L[l].n_it * L[l].nblk; L[l].dbase = db; L[l].r_first = wg * a.rpw[l];
            // unit u = blk * n_it + it (it = image * rows + row): LDS float offsets of its weight block and input block, its length
            const int x_base = l == 0 ? a.x0_off : a.xs_off;
            for (int u = tid; u < L[l].units; u += kThreads) {
                const int blk = u / L[l].n_it, it = u - blk * L[l].n_it, bi = it / r, rr = it - bi * r;
                const int g = blk / bpg, j = blk - g * bpg;
                const int len = (kg - j * kKB) < kKB ? (kg - j * kKB) : kKB;
                const int w_off = a.woff[l] + rr * Kp + g * (kg + kBlockPad * bpg) + j * (kKB + kBlockPad);
                const int x_off = x_base + bi * Kl + g * kg + j * kKB;
                desc[db + u] = make_uint2(static_cast<uint32_t>(w_off) | (static_cast<uint32_t>(x_off) << 16), static_cast<uint32_t>(len));
            }
            db += L[l].units;
            // this thread's finishing item (host guarantees B * rows-per-workgroup <= kThreads: one item per thread)
            const int items = l == last ? B * (r >> 1) : B * r, per = l == last ? (r >> 1) : r;
            if (l == last) pairs = r >> 1;
            if (tid < items) {
                L[l].fin_bi = tid / per; L[l].fin_r = tid - L[l].fin_bi * per;
                const float *bias = a.bias[l];
                if (l == last) {
                    L[l].bias0 = bias ? bias[L[l].r_first + 2 * L[l].fin_r] : 0.f;
                    L[l].bias1 = bias ? bias[L[l].r_first + 2 * L[l].fin_r + 1] : 0.f;
                    my_c = (L[l].r_first >> 1) + L[l].fin_r; my_b = L[l].fin_bi;
                } else {
                    L[l].bias0 = bias ? bias[L[l].r_first + L[l].fin_r] : 0.f;
                }
            }
        }
    }
    if (tid == 0) { s_flag[0] = 0; s_flag[1] = 1; }
    __syncthreads();
    for (int e = tid; e + 1 < a.table_len; e += kThreads)
        if (!(tab[e] < tab[e + 1])) s_flag[1] = 0;   // not strictly increasing: nearest_scale scans
    __syncthreads();
    const bool tab_sorted = s_flag[1] != 0;

    const int rw0 = L[0].rw, n_it0 = L[0].n_it, K0 = L[0].K;
    const int early_blk = (a.ntaps - 1) * a.bpg[0];      // blocks of the taps coded at least two steps ago
    const int early_units = early_blk * n_it0;
    const int late_off = (a.ntaps - 1) * C;              // the left neighbour's channels in a context window

    // ---- early window: this thread's granule pairs (tap t, channels 2 c2, 2 c2 + 1) of one image, as offsets from the window's position
    int win_rel[kWinU], win_dst[kWinU], win_tap[kWinU], win_toff[kWinU];
    {
        const int half = C >> 1, E = (a.ntaps - 1) * half;
#pragma unroll
        for (int u = 0; u < kWinU; ++u) {
            const int e = tid + u * kThreads;
            win_rel[u] = 0; win_dst[u] = 0; win_tap[u] = 63; win_toff[u] = 0;
            if (e < E) {
                const int t = e / half, c2 = e - t * half;
                win_tap[u] = t; win_toff[u] = a.tap_off[t];
                win_rel[u] = a.tap_off[t] * C + 2 * c2;
                win_dst[u] = t * C + 2 * c2;
            }
        }
    }
    // lane t of every wave keeps tap t's (dy, dx): the taps inside the image at a position become one ballot
    const int my_dy = lane < a.ntaps ? a.tap_dy[lane] : -(1 << 20), my_dx = lane < a.ntaps ? a.tap_dx[lane] : 0;

    auto dots = [&](float *out, int dbase, int u0, int u1) {
        for (int u = u0 + tid; u < u1; u += kThreads) {
            const uint2 d = desc[dbase + u];
            out[u] = block_dot_preloaded(lds + (d.x & 0xFFFFu), lds + (d.x >> 16), static_cast<int>(d.y), a.vec4);
        }
    };
    // early half of the context layer for position q -- the sums over the first early_blk blocks, in block order from zero --
    // in three pieces that need a workgroup barrier between them: the main loop runs one piece in the shadow of each of the
    // following layers' exchanges (their barriers separate the pieces); with fewer layers than pieces the rest run back to back
    auto early_piece = [&](int piece, int q) -> bool {
        bool ok = true;
        if (piece == 0) {
            const int qy = q / a.W, qx = q - qy * a.W;
            const uint64_t inside = __ballot(qy + my_dy >= 0 && qx + my_dx >= 0 && qx + my_dx < a.W);
            for (int bi = 0; bi < B; ++bi) {
                const uint64_t *base = a.yT + (static_cast<int64_t>(bi) * HW + q) * C;
                float *dst = x0 + bi * K0;
                u64x2 g[kWinU];
                bool live[kWinU];
#pragma unroll
                for (int u = 0; u < kWinU; ++u) {
                    live[u] = ((inside >> win_tap[u]) & 1ull) != 0ull;   // (tap 63: no element)
                    g[u] = u64x2{0ull, 0ull};
                    if (live[u]) g[u] = ld_gran2(base + win_rel[u]);
                }
                unsigned spins = 0;
                for (;;) {   // these positions were coded at least two steps ago: the tags match at once
                    bool all = true;
#pragma unroll
                    for (int u = 0; u < kWinU; ++u)
                        if (live[u] && !tags_are(g[u], static_cast<uint32_t>(q + win_toff[u] + 1))) { g[u] = ld_gran2(base + win_rel[u]); all = false; }
                    if (all) break;
                    if (++spins > kSpinLimit) { __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); ok = false; break; }
                }
#pragma unroll
                for (int u = 0; u < kWinU; ++u)
                    if (win_tap[u] != 63) *reinterpret_cast<f2 *>(dst + win_dst[u]) = values_of(g[u]);   // zeros outside the image
            }
        } else if (piece == 1) {
            dots(part_e, L[0].dbase, 0, early_units);
        } else {
            if (tid < n_it0) early[tid] = sum_partials(0.f, part_e + tid, n_it0, early_blk);
        }
        return ok;
    };
    auto early_pieces_from = [&](int first, int q) {   // pieces first..2, barriers in between
        for (int piece = first; piece < 3; ++piece) {
            if (piece > first) lds_barrier();
            if (!early_piece(piece, q)) *s_flag = 1;
        }
    };

    if (rw0 > 0) {
        early_pieces_from(0, 0);
        lds_barrier();
        if (*s_flag) return;
    }
    // encoder: pointers of this thread's channel of the Gaussian step, advanced by one position per step
    const bool codes = tid < B * pairs;
    const float *y_ptr = a.y ? a.y + (static_cast<int64_t>(my_b) * C + my_c) * HW : nullptr;
    float *ybuf_ptr = a.ybuf + (static_cast<int64_t>(my_b) * C + my_c) * HW;
    int32_t *sym_ptr = a.sym + static_cast<int64_t>(my_b) * C * HW + my_c, *idx_ptr = a.idx + static_cast<int64_t>(my_b) * C * HW + my_c;
    uint64_t *yT_ptr = a.yT + static_cast<int64_t>(my_b) * HW * C + my_c;

    const long long loop_c0 = a.prof ? clock64() : 0, loop_t0 = a.prof ? wall_clock64() : 0;
    int px = 0;
    bool dead = false;
    for (int p = 0; p < HW; ++p) {
        const uint32_t tag = static_cast<uint32_t>(p + 1);
        long long t0 = a.prof ? wall_clock64() : 0;
        float y_pre = 0.f;
        if (!DECODE && codes) y_pre = y_ptr[p];   // requested a whole step before it is needed
        if (rw0 > 0) {
            // ---------- context layer, late half: the left neighbour's blocks, the bias, the activation.  A row's first
            // position has no left neighbour (zeros), but the overwrite argument of the exchange buffers (header comment)
            // needs this workgroup's step p to start after position p - 1 is coded: its granules are waited for all the same.
            bool ok = true;
            for (int bi = 0; bi < B; ++bi) {
                float *dst = x0 + bi * K0 + late_off;
                if (p > 0) ok = stage_pairs(a, a.yT + (static_cast<int64_t>(bi) * HW + p - 1) * C, C >> 1, static_cast<uint32_t>(p), dst) && ok;
                if (px == 0)
                    for (int i = tid; i < (C >> 1); i += kThreads) *reinterpret_cast<f2 *>(dst + 2 * i) = f2{0.f, 0.f};
            }
            if (!ok) *s_flag = 1;
            lds_barrier();
            if (*s_flag) return;
            const long long t1 = a.prof ? wall_clock64() : 0;
            dots(part, L[0].dbase, early_units, L[0].units);
            lds_barrier();
            const long long t2 = a.prof ? wall_clock64() : 0;
            if (tid < n_it0) {
                float v = sum_partials(early[tid], part + early_units + tid, n_it0, L[0].nblk - early_blk);
                v += L[0].bias0;
                if (a.act_after[0]) v = v > 0.f ? v : 0.01f * v;   // LeakyReLU(0.01)
                st_gran(a.act[0] + static_cast<int64_t>(L[0].fin_bi) * a.rows[0] + L[0].r_first + L[0].fin_r, v, tag);
            }
            const long long t3 = a.prof ? wall_clock64() : 0;
            // ---------- early half for the next position: first piece here, in the shadow of this layer's exchange (a poisoned
            // wait shows in the flag at the next layer's barrier; with fewer than three dense layers all pieces run here)
            if (p + 1 < HW) {
                if (last >= 3) { if (!early_piece(0, p + 1)) *s_flag = 1; }
                else early_pieces_from(0, p + 1);
            }
            if (a.prof && wg == 0 && tid == 0) {
                a.prof[0] += t1 - t0; a.prof[1] += t2 - t1; a.prof[2] += t3 - t2; a.prof[3] += wall_clock64() - t3;
            }
        }
        static_for<1, kMaxLayers>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            if (l > last) return;
            const LayerRegs &R = L[l];
            const bool piece_due = rw0 > 0 && p + 1 < HW && last >= 3 && l <= 2;   // see early_piece
            if (dead) return;
            if (R.rw == 0) {   // nothing to produce here -- and nothing to wait for
                if (piece_due) { lds_barrier(); early_piece(l, p + 1); }
                return;
            }
            const long long t0 = a.prof ? wall_clock64() : 0;
            bool ok = true;
            for (int bi = 0; bi < B; ++bi) {
                float *dst = xs + bi * R.K;
                if (R.K > R.prev && a.priorT) {   // cat(ctx, prior): the prior is an input of the launch
                    const f4 *src = reinterpret_cast<const f4 *>(a.priorT + (static_cast<int64_t>(bi) * HW + p) * a.P);
                    for (int i = tid; i < ((R.K - R.prev) >> 2); i += kThreads) *reinterpret_cast<f4 *>(dst + R.prev + 4 * i) = src[i];
                }
                ok = stage_pairs(a, a.act[l - 1] + static_cast<int64_t>(bi) * R.prev, R.prev >> 1, tag, dst) && ok;
            }
            if (!ok) *s_flag = 1;
            lds_barrier();
            // a poisoned launch (some wait gave up; every later wait then fails fast) is left once per step, after a barrier:
            // at the context layer's, or here by the workgroups without context rows
            if (l == 1 && rw0 == 0 && *s_flag) { dead = true; return; }
            const long long t1 = a.prof ? wall_clock64() : 0;
            dots(part, R.dbase, 0, R.units);
            lds_barrier();
            const long long t2 = a.prof ? wall_clock64() : 0;
            if (l < last) {
                if (tid < R.n_it) {
                    float v = sum_partials(0.f, part + tid, R.n_it, R.nblk);
                    v += R.bias0;
                    if (a.act_after[l]) v = v > 0.f ? v : 0.01f * v;
                    st_gran(a.act[l] + static_cast<int64_t>(R.fin_bi) * a.rows[l] + R.r_first + R.fin_r, v, tag);
                }
                // the context layer's early half for the next position, second / third piece (see early_piece)
                if (piece_due) early_piece(l, p + 1);
            } else if (codes) {
                // ---- (mean, scale) = rows 2j, 2j + 1 ("split_interleave") summed by ONE thread, which then codes the channel
                const int i0 = R.fin_bi * R.rw + 2 * R.fin_r;
                float mu = sum_partials(0.f, part + i0, R.n_it, R.nblk), sg = sum_partials(0.f, part + i0 + 1, R.n_it, R.nblk);
                mu += R.bias0; sg += R.bias1;
                if (a.act_after[l]) { mu = mu > 0.f ? mu : 0.01f * mu; sg = sg > 0.f ? sg : 0.01f * sg; }
                const int row = nearest_scale(sg, tab, a.table_len, tab_sorted);
                if (DECODE) {
                    st_gran(a.idx_step + static_cast<int64_t>(my_b) * C + my_c, static_cast<uint32_t>(row), tag);
                    st_gran(a.mu + static_cast<int64_t>(my_b) * C + my_c, mu, tag);
                } else {
                    const float q = rintf(y_pre - mu);          // torch.round: half to even
                    st_gran(yT_ptr + static_cast<int64_t>(p) * C, q + mu, tag);   // first: every workgroup's next step waits for it
                    idx_ptr[static_cast<int64_t>(p) * C] = row;
                    sym_ptr[static_cast<int64_t>(p) * C] = static_cast<int32_t>(q);
                    ybuf_ptr[p] = q + mu;
                }
            }
            if (a.prof && wg == 0 && tid == 0) {
                a.prof[4 * l] += t1 - t0; a.prof[4 * l + 1] += t2 - t1; a.prof[4 * l + 2] += wall_clock64() - t2;
            }
        });
        if (dead) return;
        if (++px == a.W) px = 0;
    }
    if (a.prof && wg == 0 && tid == 0) {
        a.prof[4 * kMaxLayers] = clock64() - loop_c0;
        a.prof[4 * kMaxLayers + 1] = wall_clock64() - loop_t0;
    }
}

// ================================================================================================================
// Batched variant (round 4): batches of 3 .. 64 images on the matrix core.
//
// The two kernels above give a thread one (block, image, row) FMA chain: right for one or two images, 0.6 ms per coding step
// at 64.  Here the BATCH is the N dimension of v_mfma_f32_32x32x2_f32 tiles and the weights never move:
//   * a column tile = 32 images; the launch runs one independent set of `nw` compute workgroups per column tile (64 images =
//     two sets), one workgroup per compute unit;
//   * a workgroup owns ONE 32-row tile of a layer with its whole K axis, as MFMA A fragments IN REGISTERS: a wave keeps
//     eight 32-row x 64-channel blocks (256 of the 512 registers a lone wave per SIMD may use; a context tile's 36 blocks are
//     4 x 8 resident + four "late" blocks whose fragments are re-fetched each step while the wave waits anyway) -- 1.9 M
//     weights = 928 blocks fit the register files of 32 compute units, and the LDS stays free for partial tiles.  Roles: the first `nd`
//     workgroups hold row tile j of EVERY dense layer that has one (layers run one after the other, so their tiles share
//     the unit), the others one row tile of the context layer (ntaps * C / 64 blocks);
//   * a canonical block's partial tile (32 rows x 32 images) is one 32-step MFMA chain from zero -- exactly the masked
//     convolution's block (mconv.hip), so the integers agree with every other path bit for bit -- written to LDS; after a
//     workgroup barrier the 256 threads add the tile's blocks in block order (16-byte LDS reads, four outputs per thread),
//     bias, activation.  Splitting a row tile's K over workgroups would need a second exchange per layer; keeping it in one
//     compute unit costs up to three MFMA rounds per layer instead;
//   * B fragments are loaded straight from the exchange arrays into registers (lane = (k parity, image): two 256-byte runs per
//     load), validated by their tags, and fed to the chain -- no LDS staging.  All exchanged arrays are batch-minor;
//   * context layer: the taps coded at least two steps ago (all but the left neighbour) are multiplied one step AHEAD, in the
//     shadow of the dense layers; on the critical path stay C / 64 blocks and their sum.  Dense layer 1: the blocks fed by the
//     prior (an input of the launch) run before the context layer's output is waited for.
// Exchange protocol, tags, overwrite argument and bounded spins: as in the header comment (a row tile's workgroup consumes ALL
// inputs of its layer, so "produced" still implies "every input consumed").
// ================================================================================================================

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- batch-minor exchange arrays.  A [channels][nbt] slab of granules is stored in 16-byte pieces that hold the granules of
//      channels 4 m + h and 4 m + 2 + h of one column: the B operands of two consecutive MFMA steps of lane (h, column % 32), so
//      a lane fetches a block's 32 operands with sixteen 16-byte loads (each 8-byte half still validates itself by its tag).
//      Granule index of (channel c, column col):
__host__ __device__ __forceinline__ int64_t bm_gran(int c, int col, int nbt)
{
    return (static_cast<int64_t>((c >> 2) * 2 + (c & 1)) * nbt + col) * 2 + ((c >> 1) & 1);
}
//      The prior (plain floats, an input of the launch) likewise in 16-byte pieces of channels 8 m + 2 j + h, j = 0 .. 3: four steps
//      per load.  Float index of (channel c, column col) inside a position's [P][nbt] slab:
__host__ __device__ __forceinline__ int64_t bm_prior(int c, int col, int nbt)
{
    return (static_cast<int64_t>((c >> 3) * 2 + (c & 1)) * nbt + col) * 4 + ((c >> 1) & 3);
}

// A lone wave per SIMD issues one instruction per ~8-10 clocks, so a block's cost beside its 32 MFMAs (0.85 us) is its
// instruction count.  Operands are fetched with BUFFER loads: descriptor = the array, soffset (SGPR) = the block's and the piece's
// wave-uniform byte offset, voffset = the lane's constant 32-bit offset -- no vector ALU work per load, sixteen `buffer_load_dwordx4
// ... offen sc1` back to back (a `volatile` 16-byte global load would do too, but hipcc follows every volatile access with
// s_waitcnt vmcnt(0): sixteen serial round trips per block, measured 4.4 us) -- and validated with one min-tree over the 32 tags
// instead of 32 compare-and-branch pairs.  The lane offset goes through an empty asm: it keeps hipcc from treating the loads of
// different steps (same address, no store in sight) as one, and from hoisting per-load addresses out of the coding loop.
typedef __amdgpu_buffer_rsrc_t brsrc;
__device__ __forceinline__ brsrc b_rsrc(const void *p) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, 0x7FFFFFFF, 0x00020000); }
constexpr int kSc1 = 16;   // cache-policy bit of the raw buffer builtins: sc1 (agent scope: served at the L2 / memory side, never by this CU's L1)

__device__ __forceinline__ u64x2 b_ld2(brsrc r, uint32_t voff, int soff)
{
    return __builtin_bit_cast(u64x2, __builtin_amdgcn_raw_buffer_load_b128(r, static_cast<int>(voff), soff, kSc1));
}

__device__ __forceinline__ void b_issue(brsrc r, int sbase, int stride, uint32_t voff, u64x2 (&g)[16])
{
    uint32_t vo = voff;
    int sb = sbase;   // (opaque too: the sixteen scalar offsets of every block would otherwise be hoisted out of the coding loop and spilled)
    asm volatile("" : "+v"(vo), "+s"(sb)::"memory");
#pragma unroll
    for (int m = 0; m < 16; ++m) g[m] = b_ld2(r, vo, sb + m * stride);
}

// the smallest of the 32 tags: a stale granule carries an older (smaller) tag or 0, never a newer one (overwrite argument)
__device__ __forceinline__ uint32_t b_min_tag(const u64x2 (&g)[16])
{
    uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
    for (int m = 0; m < 16; ++m) mn = min(min(mn, static_cast<uint32_t>(g[m][0] >> 32)), static_cast<uint32_t>(g[m][1] >> 32));
    return mn;
}

// waits until all 32 granules carry `want` (re-issuing the block's loads while one is missing); false = poisoned launch
// (mask: the lanes whose granules are looked at -- the band schedule's lanes without a row load granules nobody publishes)
__device__ __forceinline__ bool b_wait(const ScanArgs &a, brsrc r, int sbase, int stride, uint32_t voff, uint32_t want, u64x2 (&g)[16], bool mask = true)
{
    unsigned spins = 0;
    while (__ballot(mask && b_min_tag(g) != want) != 0ull) {
        if (++spins > kSpinLimit || (spins % 256u == 0u && __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
            __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
        b_issue(r, sbase, stride, voff, g);
    }
    return true;
}

// one piece polled alone before a block's loads are issued: a wave that waits LONG (the context role, idle through the dense
// layers) keeps one load in flight instead of sixteen
__device__ __forceinline__ bool b_sentinel(const ScanArgs &a, brsrc r, int soff, uint32_t voff, uint32_t want, bool mask = true)
{
    unsigned spins = 0;
    for (;;) {
        uint32_t vo = voff;
        asm volatile("" : "+v"(vo)::"memory");
        const u64x2 g = b_ld2(r, vo, soff);
        if (__ballot(mask && min(static_cast<uint32_t>(g[0] >> 32), static_cast<uint32_t>(g[1] >> 32)) != want) == 0ull) return true;
        if (++spins > kSpinLimit || (spins % 256u == 0u && __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
            __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
    }
}

// ---- Resident weights.  The eight blocks a wave keeps for the whole launch live in the ACCUMULATOR half of the register file,
//      a[32 k + i] = A fragment i of slot k (an MFMA takes its A operand from there directly).  As a C++ array hipcc spills part of
//      it whatever the slack (its allocator treats the unified file as two halves and parks / spills around the long live ranges),
//      and a spilled weight is re-read inside the chain behind an s_waitcnt vmcnt(0).  So the 256 registers are named literally
//      (cdna_hip_programming.md 5.7 item 4): written once (b_put_weights), read only by the MFMAs below, reserved by the clobber
//      list of b_reserve_acc; EVERY MFMA of the kernel is an asm statement with its accumulator in VGPRs, so the compiler itself has
//      no use for the accumulator file -- `make audit` checks the generated code: no spill, no compiler-issued v_accvgpr_*.
//      Nothing inside an asm string is padded by the compiler: every MFMA is preceded by the two wait states a just-written B
//      operand needs, and a chain ends with the 19 states a 16-pass MFMA's result needs before anything but the next MFMA of the
//      chain touches it.
#define BASIC_A10(n) "a" #n "0", "a" #n "1", "a" #n "2", "a" #n "3", "a" #n "4", "a" #n "5", "a" #n "6", "a" #n "7", "a" #n "8", "a" #n "9"
__device__ __forceinline__ void b_reserve_acc()
{
    asm volatile("" ::: "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", BASIC_A10(1), BASIC_A10(2), BASIC_A10(3), BASIC_A10(4),
                 BASIC_A10(5), BASIC_A10(6), BASIC_A10(7), BASIC_A10(8), BASIC_A10(9), BASIC_A10(10), BASIC_A10(11), BASIC_A10(12), BASIC_A10(13),
                 BASIC_A10(14), BASIC_A10(15), BASIC_A10(16), BASIC_A10(17), BASIC_A10(18), BASIC_A10(19), BASIC_A10(20), BASIC_A10(21),
                 BASIC_A10(22), BASIC_A10(23), BASIC_A10(24), "a250", "a251", "a252", "a253", "a254", "a255");
}
#undef BASIC_A10

template <int K, int I> __device__ __forceinline__ void b_put_weights_step(const float *src, bool valid)
{
    if constexpr (I < 32) {
        const float x = valid ? src[2 * I] : 0.f;
        asm volatile("v_accvgpr_write_b32 a[%c1], %0" ::"v"(x), "n"(K * 32 + I));
        b_put_weights_step<K, I + 1>(src, valid);
    }
}
template <int K> __device__ __forceinline__ void b_put_weights(const float *src, bool valid) { b_put_weights_step<K, 0>(src, valid); }

__device__ __forceinline__ f32x16 b_zero16()
{
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}

// acc += A(slot K, fragment I) x b   /   acc += wv x b   (one v_mfma_f32_32x32x2_f32 each)
template <int K, int I> __device__ __forceinline__ void b_mfma_res(f32x16 &acc, float b)
{
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x2_f32 %0, a[%c2], %1, %0" : "+v"(acc) : "v"(b), "n"(K * 32 + I));
}
__device__ __forceinline__ void b_mfma_vgpr(f32x16 &acc, float wv, float b)
{
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x2_f32 %0, %2, %1, %0" : "+v"(acc) : "v"(b), "v"(wv));
}
__device__ __forceinline__ void b_chain_end(f32x16 &acc) { asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc)); }

// the canonical block: one MFMA chain from zero over the block's 32 channel pairs, in ascending order, A fragments = resident slot
// K, B = the block's granules.  With kRefill every piece is re-loaded from `nbase` (the block after next of this wave) as soon as
// its two MFMAs have read it: two blocks' loads are in flight or landed at any time with 128 registers of buffers
template <int K, bool kRefill, int M> __device__ __forceinline__ void b_chain_gran_step(f32x16 &acc, u64x2 (&g)[16], brsrc r, int nb, int stride, uint32_t vo)
{
    if constexpr (M < 16) {
        b_mfma_res<K, 2 * M>(acc, __uint_as_float(static_cast<uint32_t>(g[M][0])));
        b_mfma_res<K, 2 * M + 1>(acc, __uint_as_float(static_cast<uint32_t>(g[M][1])));
        if constexpr (kRefill) {
            g[M] = b_ld2(r, vo, nb + M * stride);
            __builtin_amdgcn_sched_barrier(0);   // (keeps the loads between the MFMAs: issued under the matrix pipe's 64-cycle steps)
        }
        b_chain_gran_step<K, kRefill, M + 1>(acc, g, r, nb, stride, vo);
    }
}
template <int K, bool kRefill> __device__ __forceinline__ f32x16 b_chain_gran(u64x2 (&g)[16], brsrc r, int nbase, int stride, uint32_t voff)
{
    f32x16 acc = b_zero16();
    uint32_t vo = voff;
    int nb = nbase;
    asm volatile("" : "+v"(vo), "+s"(nb)::"memory");
    b_chain_gran_step<K, kRefill, 0>(acc, g, r, nb, stride, vo);
    b_chain_end(acc);
    return acc;
}

// the same chain with A fragments and B operands both in VGPRs (a streamed block; a block fed by the prior)
template <class AF, class BF> __device__ __forceinline__ f32x16 b_chain_vv(AF &&af, BF &&bf)
{
    f32x16 acc = b_zero16();
#pragma unroll
    for (int i = 0; i < 32; ++i) b_mfma_vgpr(acc, af(i), bf(i));
    b_chain_end(acc);
    return acc;
}
template <int K, int I, class BF> __device__ __forceinline__ void b_chain_res_step(f32x16 &acc, BF &bf)
{
    if constexpr (I < 32) {
        b_mfma_res<K, I>(acc, bf(I));
        b_chain_res_step<K, I + 1>(acc, bf);
    }
}
template <int K, class BF> __device__ __forceinline__ f32x16 b_chain_res(BF &&bf)   // resident slot K, B operands from a callable
{
    f32x16 acc = b_zero16();
    b_chain_res_step<K, 0>(acc, bf);
    b_chain_end(acc);
    return acc;
}

// accumulator layout of the 32 x 32 tile: lane holds image lane % 32, rows 8 q + 4 (lane / 32) + j for register 4 q + j; the
// tile goes to LDS as [q][lane] 16-byte pieces, and thread (q, lane) of the workgroup later owns exactly those four outputs
__device__ __forceinline__ void b_store_tile(float *tile, int lane, const f32x16 &acc)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<f4 *>(tile + (q * 64 + lane) * 4) = f4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
}

// v + tile 0 + tile 1 + ... (n tiles, in that order), this thread's four outputs
__device__ __forceinline__ f4 b_sum_tiles(f4 v, const float *tiles, int n, int tid)
{
    const float *p = tiles + tid * 4;
    int b = 0;
    for (; b + 4 <= n; b += 4) {
        const f4 t0 = *reinterpret_cast<const f4 *>(p + b * kBTile), t1 = *reinterpret_cast<const f4 *>(p + (b + 1) * kBTile);
        const f4 t2 = *reinterpret_cast<const f4 *>(p + (b + 2) * kBTile), t3 = *reinterpret_cast<const f4 *>(p + (b + 3) * kBTile);
        v += t0; v += t1; v += t2; v += t3;
    }
    for (; b < n; ++b) v += *reinterpret_cast<const f4 *>(p + b * kBTile);
    return v;
}

__device__ __forceinline__ f4 b_leaky(f4 v)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v[i] > 0.f ? v[i] : 0.01f * v[i];   // LeakyReLU(0.01)
    return v;
}

// WF: the wavefront schedule (see ScanArgs; encode, and the decode of row streams -- decoder_loop, ROWS = 2): the same chains, block order, LDS sums and tag protocol; a column is a row of
// an image, a step codes one position of every row that is inside its image in that step, the slabs of the coded latent and of
// the prior are indexed by step.  Causal tap (dy, dx) of step t is column col + dy of slab t + dx + wf_s * dy (tap_off holds
// dx + wf_s * dy); a column outside its row's [0, W) publishes zero granules with the step's tag, and the pad columns in front
// of every image hold zeros for every step, so a tap outside the image multiplies zeros: no predicate inside a chain.
//
// BAND (with WF): the band schedule (encode, and the decode of row streams: the Gaussian step is then the wavefront decode launch's --
// an active slot lane publishes its table rows and means into idx_step / mu at its MFMA column for the slot's decoder wavefront,
// decoder_loop ROWS = 3, which publishes the coded granules where the encoder's lane would; everything below holds for both) --
// the wavefront's steps, slabs, taps and tags, but a lane is no longer bound to one row.
// Row r is in flight only during steps [s r, s r + W), so an image needs about W / s lanes, not H: it owns A = W / s + 1 SLOTS (lanes
// of ONE column tile, 32 / A images per tile, so the tiles of a launch share nothing and never wait for each other); slot j codes
// rows j, j + A, j + 2 A, ... back to back with period A s.  At step t the slot has u = t - s j, (n, c) = divmod(u, A s), row
// r = j + n A (before its first row: n = 0, c = u < 0) and codes (r, c) iff r < H and 0 <= c < W.  The slabs of the coded latent
// stay indexed by step and by the TRUE (image, pad + row) column, so tap (dy, dx) is still slab t + dx + s dy at column + dy,
// wave-uniform; what changes per step is the lane's own row, hence its offsets into the slabs and into y / sym / idx / ybuf, and
// the gather of the prior (transpose_prior_band_kernel).
//   * A slot "has a row" while r < H.  Such a lane publishes (slab t, row r) in EVERY step: the coded value, or zero where c lies
//     outside [0, W) -- A s > W, so every row is followed by at least one idle step of its slot.
//   * The late half's left-neighbour block reads (slab t - 1, the row the lane had in step t - 1): what the lane itself published
//     one step ago.  Inside a row that is the left neighbour; at c = 0 it is the zero of the idle step before (the padding left of
//     the image); and it is a real wait in every step, for every lane with a row -- which paces the context workgroups exactly as
//     the wavefront's columns do (overwrite argument of the header comment; the slot of the last row has a row until the last step).
//     It also validates a row's LAST granule, in the idle step that follows the row, so the early half may read every coded granule
//     unchecked as before: it was validated by this workgroup's late waves one step after it was coded, and a tap other than the
//     left neighbour is at least two steps old.
//   * Every other out-of-image tap of a coding lane lands on (slab s r' + c', row r') with c' in [-k/2, 0) or [W, W + k/2), or on a
//     pad row above the image: never coded positions, all zeros.  Who writes each: the pad rows, wavefront_pads_kernel before the
//     launch; c' in [W, A s), the row's own slot in the idle steps after the row; c' < 0 of a slot's FIRST row (r' < A), the slot
//     before it starts; the rest -- c' < 0 of rows r' >= A, and c' >= A s -- band_edges_kernel before the launch.  The two sets are
//     kept DISJOINT on purpose: a granule written before the launch would satisfy the left-neighbour wait of its slot at once, and
//     a step in which no lane of a tile really waits lets the context workgroups run ahead and overwrite layer outputs that are
//     still to be read (a latent narrower than s has such steps).
//   * A slot that has just left its last row still waits for that row's last publication (the test is "had a row one step ago"),
//     so every granule a slot publishes is validated one step later.
//   * Lanes without a row (holes of a tile, slots beyond H, slots past their last row) load from clamped in-bounds addresses, are
//     masked out of every tag test, and publish nothing into the coded latent; MFMA columns are independent, so what they compute
//     reaches nobody.  They still publish their layer outputs (slot lanes) or read the tile's first lane's (holes), so the dense
//     layers' tag tests see a published granule in every lane.
template <bool DECODE, bool WF = false, bool BAND = false>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, 1))) void scanline_batched_kernel(const ScanArgs a)
{
    static_assert(WF || !BAND, "the band schedule is a wavefront schedule");
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wg = blockIdx.x;
    if (DECODE && wg >= a.ncompute) { decoder_workgroup<WF, BAND>(a, lds); return; }
    const int HW = a.H * a.W, C = a.C, NBT = a.nbt, T = NBT >> 5;
    const int t = wg % T, j = wg / T;                  // column tile; role index inside the tile's set of workgroups
    const int h = lane >> 5, n = lane & 31, col = t * 32 + n;
    const int ncols = WF ? a.wf_cols : a.B;            // (wavefront: a column is one row of one image)
    // band: this lane's image inside its tile and its slot; a tile's first lane is always a slot of an image
    const int bA = BAND ? a.band_A : 1, bAs = bA * a.wf_s;
    const int bli = n / bA, bj = n - bli * bA;
    const bool bslot = BAND && bli < a.band_ipt && t * a.band_ipt + bli < a.B && bj < a.H;
    const bool img = BAND ? bslot : col < ncols;       // columns beyond the batch: nothing published (they LOAD the last image's
    const int colc = img ? col : (BAND ? t * 32 : ncols - 1);   // operands: no predicates, no zero fill in the load paths)
    const bool dense = j < a.nd;
    const int r0 = dense ? j : j - a.nd;               // this workgroup's row tile (dense role: of every layer that has one)
    const int nb0 = a.ntaps * a.bpt;                   // context blocks; the last kBLate run in the late half (the left neighbour's bpt among them),
    const int early = nb0 - kBLate;                    // the others -- taps coded at least two steps ago -- one step ahead
    const int frow = 8 * wave + 4 * h;                 // first of this thread's four finishing rows inside the tile
    const uint32_t voff = static_cast<uint32_t>(h * NBT + colc) * 16u;   // the lane's 16-byte piece inside a (channel quad, column tile) slab
    const int pstride = 2 * NBT * 16;                  // bytes between consecutive pieces of a lane
    // the coded latent's slabs: the same layout; the wavefront's are wf_yw columns wide (pad columns) and have their own lane offset
    // (band: the image, and the slot's FIRST row; lanes without a slot stand on row 0 of their tile's first image)
    const int wb = BAND ? (bslot ? t * a.band_ipt + bli : t * a.band_ipt) : WF ? colc / a.H : 0;
    const int wr = BAND ? (bslot ? bj : 0) : WF ? colc - wb * a.H : 0;   // wavefront: this column's image and row
    const int wpad = WF ? a.wf_s - 2 : 0;
    const int YW = WF ? a.wf_yw : NBT, ycol = WF ? wb * (a.H + wpad) + wpad + wr : colc;
    const uint32_t voff_y = WF ? static_cast<uint32_t>(h * YW + ycol) * 16u : voff;
    // band: the lane's piece inside a slab while its slot stands on row r (past the last row: clamped, the lane is masked out)
    const uint32_t voff_y0 = static_cast<uint32_t>(h * YW + ycol - wr) * 16u;
    auto band_voff = [&](int r) { return voff_y0 + static_cast<uint32_t>(r < a.H ? r : a.H - 1) * 16u; };
    // band: a slot's (column, row) one step on; it starts at (-s * slot, slot)
    auto band_step = [&](int &c, int &r) { if (++c == bAs) { c = 0; r += bA; } };
    const int ypstride = WF ? 2 * YW * 16 : pstride;
    const int nsteps = WF ? a.wf_steps : HW;
    // granule index of this thread's first finishing row (channel r0 * 32 + frow) relative to its tile's first piece
    const uint32_t soff = static_cast<uint32_t>(((frow >> 2) * 2 * NBT + col) * 2);

    // LDS: [scale table][flags][biases of this workgroup's row tiles: 3 x 32][partial tiles]
    float *tab = lds;
    int *s_flag = reinterpret_cast<int *>(lds + ((a.table_len + 3) & ~3));
    float *bias_s = lds + ((a.table_len + 3) & ~3) + 4;
    float *part = bias_s + 96;
    for (int e = tid; e < a.table_len; e += kThreads) tab[e] = a.table[e];
    if (tid < 96) {
        const int li = tid >> 5, l = dense ? 1 + li : 0;
        const float *bias = (l < a.nlayers && (dense || li == 0) && r0 < a.rt[l]) ? a.bias[l] : nullptr;
        bias_s[tid] = bias ? bias[r0 * 32 + (tid & 31)] : 0.f;
    }
    if (tid == 0) s_flag[1] = 1;
    __syncthreads();
    for (int e = tid; e + 1 < a.table_len; e += kThreads)
        if (!(tab[e] < tab[e + 1])) s_flag[1] = 0;   // not strictly increasing: nearest_scale scans
    __syncthreads();
    const bool tab_sorted = s_flag[1] != 0;

    // ---- this wave's resident weight blocks: A fragments (lane = row lane % 32 of the tile, channel parity lane / 32) in the
    // accumulator file, see b_put_weights
    b_reserve_acc();
    static_for<0, kBSlots>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        constexpr int l = 1 + k / kBDenseSlots;                      // dense role: the slot's layer and block
        const int b = wave + 4 * (k % kBDenseSlots), e = wave + 4 * k;   // context role: its early block
        const bool v = dense ? (l < a.nlayers && r0 < a.rt[l] && b < a.nblk[l]) : e < early;   // wave-uniform
        const int li = dense ? (l < a.nlayers ? l : 0) : 0;
        b_put_weights<k>(a.w[li] + static_cast<int64_t>(r0 * 32 + n) * a.kdim[li] + 64 * (dense ? b : e) + h, v);
    });
    asm volatile("s_nop 4" ::: "memory");   // (accumulator writes -> the first MFMA that reads them)
    const f4 zero4 = f4{0.f, 0.f, 0.f, 0.f};
    u64x2 gA[16], gB[16];

    // publishes this thread's four finishing rows of its tile into a [rows][nbt] exchange slab (tile = slab + the tile's first piece)
    auto publish4 = [&](uint64_t *tile, const f4 &v, uint32_t tag) {
        if (!img) return;
        uint32_t so = soff;
        asm volatile("" : "+v"(so));   // (or the four addresses are hoisted out of the coding loop and spilled)
#pragma unroll
        for (int i = 0; i < 4; ++i) st_gran(tile + (so + static_cast<uint32_t>((i & 1) * 2 * NBT + (i >> 1))), v[i], tag);
    };

    if (!dense) {
        // ================= context role: row tile r0 of the masked context convolution =================
        const char *yT8 = reinterpret_cast<const char *>(a.yT);
        const int blk_bytes = 16 * ypstride;   // a 64-channel block of a slab
        uint64_t *out_tile = a.act[0] + static_cast<int64_t>(r0 * 8) * 2 * NBT * 2;
        const int64_t pos_bytes = static_cast<int64_t>(C) * YW * 8;   // a position's (wavefront: a step's) slab of the coded latent
        f4 esum = zero4;   // position 0 has no causal neighbour: its early sum is zero
        int px = 0, py = 0;
        int b_c = -a.wf_s * wr, b_r = wr, b_rp = wr;   // band: this slot's column and row in step p, its row in step p - 1
        // this wave's late block as A fragments, lane-major (8 x 16 bytes per lane): saved once, re-fetched every step
        const char *wfrag = reinterpret_cast<const char *>(a.wlate) + static_cast<int64_t>(wg) * (kThreads * 128);
        {
            const int e = early + wave;
            const float *src = a.w[0] + static_cast<int64_t>(r0 * 32 + n) * a.kdim[0] + 64 * e + h;
            float *dst = reinterpret_cast<float *>(const_cast<char *>(wfrag)) + tid * 32;
#pragma unroll
            for (int i = 0; i < 32; ++i) dst[i] = src[2 * i];
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const bool prof1 = a.prof && wg == a.nd * T && tid == 64, prof0 = a.prof && wg == a.nd * T && tid == 0;   // BASIC_SCAN_PROFILE: first context workgroup, waves 1 / 0
        const long long loop_t0 = prof0 ? wall_clock64() : 0;
        for (int p = 0; p < nsteps; ++p) {
            const uint32_t tag = static_cast<uint32_t>(p + 1);
            const long long tp0 = a.prof ? wall_clock64() : 0;
            long long tp1 = tp0;
            // ---------- late half: the last four blocks of the K axis, one per wave.  The left neighbour's (the last tap's) need
            // position p - 1, coded a moment ago: sentinel, then tags.  A row's first position has no left neighbour (zeros), but
            // the overwrite argument of the exchange arrays needs this step to start after position p - 1 is coded: its granules
            // are waited for all the same.  The block's weights come from this wave's fragment copy, requested before the wait
            {
                const int e = early + wave, tp = e / a.bpt, cb = e - tp * a.bpt;
                const bool left = tp == a.ntaps - 1;
                // wavefront: the tap's slab is a step (left: p - 1 as well); before step 0 it is outside the image for every column
                const int ny = py + a.tap_dy[tp], nx = px + a.tap_dx[tp];
                const bool inside = WF ? p + a.tap_off[tp] >= 0 : ny >= 0 && nx >= 0 && nx < a.W;
                const int dyb = WF ? a.tap_dy[tp] * 16 : 0;   // wavefront: the tap's row is the column dy pieces further on
                // band: the left neighbour's block reads what this lane published one step ago, the others stand on this step's row;
                // looked at are the lanes that had a row one step ago (left) / that code a position in this step (see the band section)
                const bool b_has = bslot && b_r < a.H;
                const uint32_t vyl = BAND ? band_voff(left ? b_rp : b_r) : voff_y;
                const bool ml = !BAND || (left ? bslot && b_rp < a.H : b_has && static_cast<unsigned>(b_c) < static_cast<unsigned>(a.W));
                f4 wl4[8];
                {
                    uint32_t fo = static_cast<uint32_t>(tid) * 128u;
                    asm volatile("" : "+v"(fo)::"memory");
#pragma unroll
                    for (int m = 0; m < 8; ++m) wl4[m] = *reinterpret_cast<const f4 *>(wfrag + (fo + static_cast<uint32_t>(m * 16)));
                }
                f32x16 acc = b_zero16();
                if (inside || (left && p > 0)) {
                    const int pos = left ? p - 1 : p + a.tap_off[tp];
                    const brsrc yr = b_rsrc(yT8 + pos * pos_bytes + dyb);
                    const int sb = cb * blk_bytes;
                    if (left && !b_sentinel(a, yr, sb + 15 * ypstride, vyl, static_cast<uint32_t>(pos + 1), ml)) return;
                    if (a.prof) tp1 = wall_clock64();
                    b_issue(yr, sb, ypstride, vyl, gA);
                    if (!b_wait(a, yr, sb, ypstride, vyl, static_cast<uint32_t>(pos + 1), gA, ml)) return;
                    if (inside)
                        acc = b_chain_vv([&](int i) { return wl4[i >> 2][i & 3]; }, [&](int i) { return __uint_as_float(static_cast<uint32_t>(gA[i >> 1][i & 1])); });
                }
                b_store_tile(part + e * kBTile, lane, acc);
            }
            const long long tp2 = a.prof ? wall_clock64() : 0;
            lds_barrier();
            {
                f4 v = b_sum_tiles(esum, part + early * kBTile, kBLate, tid);
                v += *reinterpret_cast<const f4 *>(bias_s + frow);
                if (a.act_after[0]) v = b_leaky(v);
                publish4(out_tile, v, tag);
            }
            const long long tp3 = a.prof ? wall_clock64() : 0;
            if (prof1) { a.prof[0] += tp1 - tp0; a.prof[1] += tp2 - tp1; a.prof[2] += tp3 - tp2; }
            if (!WF && ++px == a.W) { px = 0; ++py; }
            if constexpr (BAND) { b_rp = b_r; band_step(b_c, b_r); }
            if (p + 1 == nsteps) break;
            // ---------- early half for the next position q = p + 1, in the shadow of the dense layers: partial tiles of the blocks
            // of the taps coded at least two steps ago, then their sum in block order.  Every granule read here was validated by
            // this workgroup's late waves in an earlier step (the newest, position p - 1, in this step's late half, before the
            // barrier above), so the tags are not looked at again.  Two buffers: while block k's chain runs, its buffer is
            // re-filled piece by piece with block k + 2 (the loads sit between the MFMAs, where a lone wave's issue slots are
            // free), block k + 1 landed during the chain before
            const int q = p + 1, qy = py, qx = px;
            const uint32_t vye = BAND ? band_voff(b_r) : voff_y;   // (band: the lane's piece on the row its slot has in step q)
            auto early_valid = [&](int kk) { return wave + 4 * kk < early; };
            // block e of this position's early window: false when its tap lies outside the image (zeros); r / sb = where its operands are
            auto early_src = [&](int e, brsrc &r, int &sb) -> bool {
                const int tp = e / a.bpt, cb = e - tp * a.bpt;
                const int ny = qy + a.tap_dy[tp], nx = qx + a.tap_dx[tp];
                const bool inside = WF ? q + a.tap_off[tp] >= 0 : ny >= 0 && nx >= 0 && nx < a.W;
                r = b_rsrc(yT8 + (inside ? q + a.tap_off[tp] : q - 1) * pos_bytes + (WF ? a.tap_dy[tp] * 16 : 0));   // (outside: any coded position -- loaded into a buffer nobody reads)
                sb = cb * blk_bytes;
                return inside;
            };
            // Wavefront, second column tile: a tap of a row above reads, in this tile's first lanes, columns of the OTHER tile, which
            // this workgroup's late waves never validated (the tile sets run independently) -- those blocks wait for their tags
            // here.  (Pad columns are written before the launch; columns of this tile: the argument above.)
            auto early_tag = [&](int e, uint32_t &want) -> bool {
                const int tp = e / a.bpt;
                want = static_cast<uint32_t>(q + a.tap_off[tp] + 1);
                return WF && !BAND && t > 0 && a.tap_dy[tp] != 0;   // (band: an image's slots share a tile)
            };
            bool early_ok = true;
            bool have_a = false, have_b = false;   // whether buffer A / B holds (or is receiving) a block that is used
            {
                brsrc r; int sb;
                if (early_valid(0) && (have_a = early_src(wave, r, sb))) b_issue(r, sb, ypstride, vye, gA);
                if (early_valid(1) && (have_b = early_src(wave + 4, r, sb))) b_issue(r, sb, ypstride, vye, gB);
            }
            static_for<0, kBSlots>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                if (!early_valid(k)) return;
                u64x2(&cur)[16] = *((k & 1) ? &gB : &gA);
                bool &have_cur = (k & 1) ? have_b : have_a;
                brsrc r2 = b_rsrc(yT8);
                int sb2 = 0;
                const bool next = k + 2 < kBSlots && early_valid(k + 2);
                const bool have_next = next && early_src(wave + 4 * (k + 2), r2, sb2);
                f32x16 acc = b_zero16();
                if (have_cur) {
                    if constexpr (WF) {
                        uint32_t want;
                        if (early_tag(wave + 4 * k, want)) {
                            brsrc rc = b_rsrc(yT8);
                            int sbc = 0;
                            early_src(wave + 4 * k, rc, sbc);
                            early_ok = b_wait(a, rc, sbc, ypstride, vye, want, cur) && early_ok;
                        }
                    }
                    if (!next) early_src(wave + 4 * k, r2, sb2);   // nothing follows: the refill re-reads this block (no second copy of the chain)
                    acc = b_chain_gran<k, true>(cur, r2, sb2, ypstride, vye);
                } else if (have_next) {
                    b_issue(r2, sb2, ypstride, vye, cur);   // (a tap outside the image enters as zeros: no chain to hide the loads behind)
                }
                have_cur = have_next;
                b_store_tile(part + (wave + 4 * k) * kBTile, lane, acc);
            });
            if (WF && !early_ok) return;
            lds_barrier();
            esum = b_sum_tiles(zero4, part, early, tid);
            if (prof0) a.prof[3] += wall_clock64() - tp3;
        }
        if (prof0) a.prof[4 * kMaxLayers + 2] = wall_clock64() - loop_t0;
        return;
    }

    // ================= dense role: row tile r0 of every dense layer that has one =================
    const int last = a.nlayers - 1;
    const bool codes = r0 < a.rt[last] && img;     // this thread finishes two (mean, scale) pairs of image `col`
    const int c0 = (r0 * 32 + frow) >> 1;          // its channels c0, c0 + 1  (rows 2c = mean, 2c + 1 = scale: "split_interleave")
    // element offsets of (image col, channel c0) in y / ybuf [B][C][HW], sym / idx [B][HW * C], the coded latent's slab, mu / idx_step [nbt][C]
    // (wavefront: of (image wb, channel c0, first position of row wr); the row's position of the step is added per step)
    // (band: of (image wb, channel c0, position 0) and of the image's row 0; the slot's row and column of the step are added per step)
    const uint32_t yoff = static_cast<uint32_t>(BAND ? (wb * C + c0) * HW : WF ? (wb * C + c0) * HW + wr * a.W : (col * C + c0) * HW);
    const uint32_t ooff = static_cast<uint32_t>(BAND ? wb * HW * C + c0 : WF ? (wb * HW + wr * a.W) * C + c0 : col * C * HW + c0);
    const uint32_t toff = static_cast<uint32_t>(bm_gran(c0, BAND ? ycol - wr : WF ? ycol : col, YW)), moff = static_cast<uint32_t>(col * C + c0);
    const int wsr = WF ? a.wf_s * wr : 0;              // wavefront: the step in which this column's row starts
    int b_c = -wsr, b_r = wr;                          // band: this slot's column and row in step p
    const bool prof = a.prof && wg == 0 && tid == 0;   // BASIC_SCAN_PROFILE: first dense workgroup, wave 0
    const long long loop_c0 = prof ? clock64() : 0, loop_t0 = prof ? wall_clock64() : 0;
    for (int p = 0; p < nsteps; ++p) {
        const uint32_t tag = static_cast<uint32_t>(p + 1);
        // wavefront: the column position this lane's row codes in this step; outside [0, W) the column is idle (zeros published)
        const int wc = BAND ? b_r * a.W + b_c : WF ? p - wsr : 0;   // (band: the position inside the image)
        const bool b_has = !BAND || (bslot && b_r < a.H);           // band: the slot has a row in this step
        const bool active = !WF || (b_has && static_cast<unsigned>(BAND ? b_c : wc) < static_cast<unsigned>(a.W));
        const uint32_t b_to = BAND ? static_cast<uint32_t>(2 * (b_r < a.H ? b_r : a.H - 1)) : 0u;   // band: the row's column inside a slab
        if constexpr (BAND) band_step(b_c, b_r);
        // (per-thread element offsets stay 32-bit and opaque: as 64-bit addresses hoisted out of the loop they would be spilled)
        float y_pre0 = 0.f, y_pre1 = 0.f;
        if (!DECODE && codes && active) {   // requested a whole step before they are needed
            uint32_t yo = yoff;
            asm volatile("" : "+v"(yo));
            if constexpr (WF) yo += static_cast<uint32_t>(wc);
            y_pre0 = (a.y + (WF ? 0 : p))[yo];
            y_pre1 = (a.y + (WF ? 0 : p))[yo + static_cast<uint32_t>(HW)];
        }
        bool alive = true;
        static_for<1, 4>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            if (l > last || r0 >= a.rt[l] || !alive) return;
            float *tiles = part + a.tile_off[l];
            const int fed = l == 1 ? a.ctx_blocks : a.nblk[l];   // blocks fed by the previous layer; the rest (layer 1): the prior
            const long long tq0 = a.prof ? wall_clock64() : 0;
            // (1) the prior's blocks: inputs of the launch, nothing to wait for (16-byte pieces of four steps' operands)
            if (l == 1) {
                static_for<0, kBDenseSlots>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    const int b = wave + 4 * k;
                    if (b < fed || b >= a.nblk[1]) return;
                    const brsrc pr = b_rsrc(reinterpret_cast<const char *>(a.priorT) + static_cast<int64_t>(p) * a.P * NBT * 4);
                    int sb = 8 * (b - fed) * pstride;
                    f4 pv[8];
                    uint32_t vo = voff;
                    asm volatile("" : "+v"(vo), "+s"(sb)::"memory");
#pragma unroll
                    for (int m = 0; m < 8; ++m) pv[m] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(pr, static_cast<int>(vo), sb + m * pstride, 0));
                    const f32x16 acc = b_chain_res<k>([&](int i) { return pv[i >> 2][i & 3]; });
                    b_store_tile(tiles + b * kBTile, lane, acc);
                });
            }
            // (2) the blocks fed by layer l - 1: the first two blocks' loads go out together, the third's piece by piece behind the first
            // chain's MFMAs (no sentinel: the producers are rarely behind, and a second round trip per layer costs more than the polling)
            const long long tq1 = a.prof ? wall_clock64() : 0;
            const brsrc xr = b_rsrc(a.act[l - 1]);
            const int nb = wave < fed ? (fed - wave + 3) >> 2 : 0;   // this wave's blocks wave, wave + 4, wave + 8 below `fed`
            const int b0 = 16 * wave * pstride, b1 = b0 + 64 * pstride, b2 = b1 + 64 * pstride;   // their byte offsets in the slab
            if (nb >= 1) b_issue(xr, b0, pstride, voff, gA);
            if (nb >= 2) b_issue(xr, b1, pstride, voff, gB);
            if (nb >= 1) {
                alive = b_wait(a, xr, b0, pstride, voff, tag, gA) && alive;
                const f32x16 acc = (nb >= 3 && (l - 1) * kBDenseSlots + 2 < kBSlots) ? b_chain_gran<(l - 1) * kBDenseSlots, true>(gA, xr, b2, pstride, voff)
                                                                                    : b_chain_gran<(l - 1) * kBDenseSlots, false>(gA, xr, 0, 0, 0u);
                b_store_tile(tiles + wave * kBTile, lane, acc);
            }
            if (nb >= 2) {
                alive = b_wait(a, xr, b1, pstride, voff, tag, gB) && alive;
                const f32x16 acc = b_chain_gran<(l - 1) * kBDenseSlots + 1, false>(gB, xr, 0, 0, 0u);
                b_store_tile(tiles + (wave + 4) * kBTile, lane, acc);
            }
            if constexpr ((l - 1) * kBDenseSlots + 2 < kBSlots) {   // (the last layer has two register slots per wave)
                if (nb >= 3) {
                    alive = b_wait(a, xr, b2, pstride, voff, tag, gA) && alive;
                    const f32x16 acc = b_chain_gran<(l - 1) * kBDenseSlots + 2, false>(gA, xr, 0, 0, 0u);
                    b_store_tile(tiles + (wave + 8) * kBTile, lane, acc);
                }
            }
            if (!alive) return;
            const long long tq2 = a.prof ? wall_clock64() : 0;
            lds_barrier();
            f4 v = b_sum_tiles(zero4, tiles, a.nblk[l], tid);
            v += *reinterpret_cast<const f4 *>(bias_s + (l - 1) * 32 + frow);
            if (a.act_after[l]) v = b_leaky(v);
            if (l < last) {
                publish4(a.act[l] + static_cast<int64_t>(r0 * 8) * 2 * NBT * 2, v, tag);
            } else if (img) {
                // ---- Gaussian step: this thread's two (mean, scale) pairs.  What the next step waits for goes out first: the coded
                // latent (encoder) -- the table search and the plain outputs follow in its shadow
                uint32_t yo = yoff, oo = ooff, to = toff, mo = moff;
                asm volatile("" : "+v"(yo), "+v"(oo), "+v"(to), "+v"(mo));
                uint64_t *ypos = a.yT + static_cast<int64_t>(p) * C * YW;
                if constexpr (BAND) to += b_to;
                if (WF && !active) {   // an idle column: the zero padding left and right of its row (band: of a slot with a row) -- in
                    if (b_has) {       // a decode launch too: the row's decoder wavefront publishes the row's own positions only
                        st_gran(ypos + to, 0.f, tag);
                        st_gran(ypos + (to + static_cast<uint32_t>(2 * YW)), 0.f, tag);
                    }
                } else if (DECODE) {   // (wavefront: mu / idx_step are indexed by column, and so read by the column's decoder wavefronts)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int row = nearest_scale(v[2 * i + 1], tab, a.table_len, tab_sorted);
                        st_gran(a.idx_step + (mo + i), static_cast<uint32_t>(row), tag);
                        st_gran(a.mu + (mo + i), v[2 * i], tag);
                    }
                } else {
                    const float q0 = rintf(y_pre0 - v[0]), q1 = rintf(y_pre1 - v[2]);          // torch.round: half to even
                    st_gran(ypos + to, q0 + v[0], tag);
                    st_gran(ypos + (to + static_cast<uint32_t>(2 * YW)), q1 + v[2], tag);     // channel c0 + 1: the odd-parity piece of the same quad
                    const int op = WF ? 0 : p;
                    if constexpr (WF) { oo += static_cast<uint32_t>(wc * C); yo += static_cast<uint32_t>(wc); }
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const float mu = v[2 * i], qq = i ? q1 : q0;
                        const int row = nearest_scale(v[2 * i + 1], tab, a.table_len, tab_sorted);
                        (a.idx + static_cast<int64_t>(op) * C)[oo + i] = row;
                        (a.sym + static_cast<int64_t>(op) * C)[oo + i] = static_cast<int32_t>(qq);
                        (a.ybuf + op)[yo + static_cast<uint32_t>(i * HW)] = qq + mu;
                    }
                }
            }
            if (prof) { a.prof[4 * l] += tq1 - tq0; a.prof[4 * l + 1] += tq2 - tq1; a.prof[4 * l + 2] += wall_clock64() - tq2; }
        });
        if (!alive) return;
        lds_barrier();   // a layer's partial tiles are rewritten in the next step (a workgroup with one layer has no other barrier in between)
    }
    if (prof) {
        a.prof[4 * kMaxLayers] = clock64() - loop_c0;
        a.prof[4 * kMaxLayers + 1] = wall_clock64() - loop_t0;
    }
}

// prior [B][P][HW] -> priorT [HW] x slab [P][nbt] in 16-byte pieces of four steps' operands (bm_prior)
__global__ void transpose_prior_batched_kernel(const float *__restrict__ in, float *__restrict__ out, int B, int P, int HW, int nbt, int64_t total)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int p = static_cast<int>(i % HW);   // position fastest: coalesced reads
        const int64_t r = i / HW;
        const int c = static_cast<int>(r % P);
        const int b = static_cast<int>(r / P);
        out[static_cast<int64_t>(p) * P * nbt + bm_prior(c, b, nbt)] = in[i];
    }
}

// wavefront schedule: prior [B][P][HW] -> priorT [steps] x slab [P][nbt] (bm_prior), column b * H + r of step t = position
// (r, t - s * r) of image b, zero where that lies outside the row (the column is idle in that step)
__global__ void transpose_prior_wavefront_kernel(const float *__restrict__ in, float *__restrict__ out, int P, int H, int W, int s, int steps, int nbt,
                                                 int64_t total)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int t = static_cast<int>(i % steps);   // step fastest: a row's positions, coalesced reads
        const int64_t q = i / steps;
        const int c = static_cast<int>(q % P);
        const int col = static_cast<int>(q / P), b = col / H, r = col - b * H;
        const int x = t - s * r;
        out[static_cast<int64_t>(t) * P * nbt + bm_prior(c, col, nbt)] = (x >= 0 && x < W) ? in[(static_cast<int64_t>(b) * P + c) * H * W + r * W + x] : 0.f;
    }
}

// wavefront schedule: the pad columns of every step's slab of the coded latent (the rows above each image): granules { 0.0f, step + 1 },
// constants of the launch, written in stream order before it (the rest of the array is zeroed: tag 0)
__global__ void wavefront_pads_kernel(uint64_t *__restrict__ yT, int C, int B, int H, int pad, int yw, int64_t total)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int k = static_cast<int>(i % pad);
        int64_t q = i / pad;
        const int b = static_cast<int>(q % B);
        q /= B;
        const int c = static_cast<int>(q % C);
        const int64_t t = q / C;
        yT[t * C * yw + bm_gran(c, b * (H + pad) + k, yw)] = static_cast<uint64_t>(t + 1) << 32;
    }
}

// band schedule: prior [B][P][HW] -> priorT [steps] x slab [P][nbt] (bm_prior); lane column (tile, lane) of step t = the position its
// slot codes in that step, zero where it codes none (all nbt columns are written: a hole lane reads its tile's first column)
__global__ void transpose_prior_band_kernel(const float *__restrict__ in, float *__restrict__ out, int P, int B, int H, int W, int s, int A, int ipt,
                                            int steps, int nbt, int64_t total)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int t = static_cast<int>(i % steps);   // step fastest: a row's positions, coalesced reads
        const int64_t q = i / steps;
        const int c = static_cast<int>(q % P);
        const int col = static_cast<int>(q / P), n = col & 31, li = n / A, j = n - li * A, b = (col >> 5) * ipt + li;
        const int u = t - s * j;
        float v = 0.f;
        if (li < ipt && b < B && j < H && u >= 0) {
            const int k = u / (A * s), x = u - k * (A * s), r = j + k * A;
            if (r < H && x < W) v = in[(static_cast<int64_t>(b) * P + c) * H * W + r * W + x];
        }
        out[static_cast<int64_t>(t) * P * nbt + bm_prior(c, col, nbt)] = v;
    }
}

// band schedule: the padding left and right of every row -- granules (slab s * r + x, row r) for x in [-pad, 0) and [W, W + pad), as far
// as the slab exists and NO slot publishes the granule during the launch (x < 0: rows r >= A; x >= W: x >= A * s; see the band
// section): { 0.0f, slab + 1 }, never a coded position (wavefront_pads_kernel writes the rows above the image)
__global__ void band_edges_kernel(uint64_t *__restrict__ yT, int C, int B, int H, int W, int s, int A, int pad, int steps, int yw, int64_t total)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int k = static_cast<int>(i % (2 * pad));
        int64_t q = i / (2 * pad);
        const int r = static_cast<int>(q % H);
        q /= H;
        const int b = static_cast<int>(q % B);
        const int c = static_cast<int>(q / B);
        const int x = k < pad ? k - pad : W + k - pad;
        const int64_t slab = static_cast<int64_t>(s) * r + x;
        if ((x < 0 ? r >= A : x >= A * s) && slab >= 0 && slab < steps) yT[slab * C * yw + bm_gran(c, b * (H + pad) + pad + r, yw)] = static_cast<uint64_t>(slab + 1) << 32;
    }
}

// prior [B][P][HW] -> priorT [B][HW][P]
__global__ void transpose_prior_kernel(const float *__restrict__ in, float *__restrict__ out, int P, int HW, int64_t total)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int c = static_cast<int>(i % P);
        const int64_t r = i / P;
        const int p = static_cast<int>(r % HW);
        const int64_t b = r / HW;
        out[i] = in[(b * P + c) * HW + p];
    }
}

}  // namespace

// The integer geometry (scan_plan.h) plus the device state
struct basic_scanline_plan : ScanGeometry {
    explicit basic_scanline_plan(const ScanGeometry &g) : ScanGeometry(g) {}
    float *d_w[kMaxLayers] = {}, *d_b[kMaxLayers] = {};
    // per-call scratch (grow-only): exchange buffers, position-major copies of the coded latent and the prior, step buffers
    float *d_scratch = nullptr;
    size_t scratch_cap = 0;
    unsigned *d_bar = nullptr;   // [0] barrier counter, [1] error flag
    hipEvent_t done = nullptr;   // completion of this plan's last launch (see ScanChain)
    int encode_schedule = BASIC_SCAN_SCHEDULE_AUTO;   // basic_scanline_set_encode_schedule
    int decode_schedule = BASIC_SCAN_SCHEDULE_AUTO;   // basic_scanline_set_decode_schedule: row-stream decode calls only
    int last_kernel = BASIC_SCAN_KERNEL_NONE;         // basic_scanline_last_kernel
};

namespace {

// Persistent launches spin on a device-wide barrier and must be fully resident (one workgroup per compute unit), so grids
// started from different HIP streams (concurrent stream workers) could each hold compute units the other is waiting for
// until both give up.  They are therefore admitted in GPU time, in host enqueue order: the chip is cut into three slots of
// CUs / 3 compute units; a launch of G workgroups takes ceil(G / (CUs / 3)) consecutive slots (round robin), waits -- a
// stream-wait, nothing blocks on the host -- for the launches that last held them and leaves its own completion event
// there.  Launches in flight hold disjoint slots, so together they never need more compute units than the chip has.
// Ordinary kernels of other streams are no hazard: they drain, and the barrier's spin bound (seconds) covers the wait.
struct ScanChain {
    std::mutex mu;
    struct Dev { hipEvent_t slot[3] = {nullptr, nullptr, nullptr}; int cursor = 0; };
    Dev dev[16];   // per device: launches on different GPUs of one process share nothing (they used to wait on each other's events)
};
ScanChain g_scan_chain;

template <typename Launch> int chained_launch(basic_scanline_plan *p, hipStream_t st, int grid, int cus, Launch &&launch)
{
    int device = 0;
    BASIC_HIP_TRY(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_scan_chain.mu);
    ScanChain::Dev &d = g_scan_chain.dev[device & 15];
    if (!p->done) BASIC_HIP_TRY(hipEventCreateWithFlags(&p->done, hipEventDisableTiming));
    const int per_slot = cus / 3 > 0 ? cus / 3 : 1;
    const int need = std::min(3, (grid + per_slot - 1) / per_slot);
    for (int j = 0; j < need; ++j) {
        hipEvent_t e = d.slot[(d.cursor + j) % 3];
        if (e && e != p->done) BASIC_HIP_TRY(hipStreamWaitEvent(st, e, 0));   // (its own previous launch: same stream, already ordered)
    }
    launch();
    BASIC_HIP_TRY(hipGetLastError());
    BASIC_HIP_TRY(hipEventRecord(p->done, st));
    for (int j = 0; j < need; ++j) d.slot[(d.cursor + j) % 3] = p->done;
    d.cursor = (d.cursor + need) % 3;
    return BASIC_OK;
}

}  // namespace

extern "C" void basic_scanline_plan_destroy(basic_scanline_plan *p)
{
    if (!p) return;
    for (int l = 0; l < kMaxLayers; ++l) {
        if (p->d_w[l]) (void)hipFree(p->d_w[l]);
        if (p->d_b[l]) (void)hipFree(p->d_b[l]);
    }
    if (p->d_scratch) (void)hipFree(p->d_scratch);
    if (p->d_bar) (void)hipFree(p->d_bar);
    if (p->done) {
        std::lock_guard<std::mutex> lock(g_scan_chain.mu);
        for (auto &d : g_scan_chain.dev)
            for (int i = 0; i < 3; ++i)
                if (d.slot[i] == p->done) {
                    (void)hipEventSynchronize(p->done);   // whoever waits on it has been released
                    d.slot[i] = nullptr;
                }
        (void)hipEventDestroy(p->done);
    }
    delete p;
}

extern "C" int basic_scanline_plan_create(const float *ctx_weight, const float *ctx_bias, int channels, int ctx_out, int ksize,
                                          int prior_channels, int n_dense, const float *const *dense_weight,
                                          const float *const *dense_bias, const int *dense_out, const int *act_after,
                                          const int *dense_in_groups, basic_scanline_plan **out)
{
    int rc = require_device();
    if (rc) return rc;
    BASIC_REQUIRE(ctx_weight && out && dense_weight, "scanline_plan_create: bad argument");
    ScanGeometry g;
    rc = scan_geometry(channels, ctx_out, ksize, prior_channels, n_dense, dense_out, act_after, dense_in_groups, &g);
    if (rc) return rc;
    auto *p = new basic_scanline_plan(g);
    const int half = ksize / 2;
    // upload: context weights as [row][tap][c] (only the causal taps), dense layers as they are ([rows][k]); padded by
    // one workgroup's worth of rows so that the slice copy of the last workgroup never reads past the buffer
    auto upload = [&](const std::vector<float> &h, float **d) -> int {
        BASIC_HIP_TRY(hipMalloc(d, h.size() * sizeof(float)));
        BASIC_HIP_TRY(hipMemcpy(*d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        return BASIC_OK;
    };
    {
        std::vector<float> h(static_cast<size_t>(p->rows[0] + p->rpw[0]) * p->kdim[0], 0.f);
        for (int r = 0; r < ctx_out; ++r)
            for (int t = 0; t < p->ntaps; ++t)
                for (int c = 0; c < channels; ++c)
                    h[(static_cast<size_t>(r) * p->ntaps + t) * channels + c] =
                        ctx_weight[((static_cast<size_t>(r) * channels + c) * ksize + (p->tap_dy[t] + half)) * ksize + (p->tap_dx[t] + half)];
        rc = upload(h, &p->d_w[0]);
        if (!rc && ctx_bias) { std::vector<float> hb(ctx_bias, ctx_bias + ctx_out); hb.resize(ctx_out + p->rpw[0], 0.f); rc = upload(hb, &p->d_b[0]); }
    }
    for (int l = 1; l <= n_dense && !rc; ++l) {
        std::vector<float> h(static_cast<size_t>(p->rows[l] + p->rpw[l]) * p->kdim[l], 0.f);
        std::copy(dense_weight[l - 1], dense_weight[l - 1] + static_cast<size_t>(p->rows[l]) * p->kdim[l], h.begin());
        rc = upload(h, &p->d_w[l]);
        if (!rc && dense_bias && dense_bias[l - 1]) {
            std::vector<float> hb(dense_bias[l - 1], dense_bias[l - 1] + p->rows[l]);
            hb.resize(p->rows[l] + p->rpw[l], 0.f);
            rc = upload(hb, &p->d_b[l]);
        }
    }
    if (!rc) {
        hipError_t e = hipMalloc(&p->d_bar, 2 * sizeof(unsigned));
        if (e != hipSuccess) rc = hip_fail(e, "scanline_plan_create", __FILE__, __LINE__);
    }
    if (rc) { basic_scanline_plan_destroy(p); return rc; }
    *out = p;
    return BASIC_OK;
}

extern "C" int basic_scanline_plan_info(const basic_scanline_plan *p, int *workgroups, int *lds_weight_bytes)
{
    BASIC_REQUIRE(p, "scanline_plan_info: null plan");
    if (workgroups) *workgroups = p->nwg;
    if (lds_weight_bytes) *lds_weight_bytes = p->weight_floats * static_cast<int>(sizeof(float));
    return BASIC_OK;
}

namespace {

// ---- The persistent kernels: what needs HIP of the list that scan_plan.h owns (kScanKernelNames: ids and environment spellings), row for row
using ScanFn = void (*)(ScanArgs);
struct ScanKernelRow {
    const char *label;   // ScanProfile
    ScanFn fn;           // (the wavefront's and the band's decode rows serve row-stream calls only: scan_kernel_decodes)
};
template <bool DECODE> constexpr ScanKernelRow kScanKernels[] = {
    {DECODE ? "decode (band)" : "encode (band)", scanline_batched_kernel<DECODE, true, true>},
    {DECODE ? "decode (wavefront)" : "encode (wavefront)", scanline_batched_kernel<DECODE, true>},
    {DECODE ? "decode (batched)" : "encode (batched)", scanline_batched_kernel<DECODE>},
    {DECODE ? "decode" : "encode", scanline_pipelined_kernel<DECODE>},
    {DECODE ? "decode" : "encode", scanline_persistent_kernel<DECODE>},
};
static_assert(sizeof(kScanKernels<false>) / sizeof(ScanKernelRow) == sizeof(kScanKernelNames) / sizeof(ScanKernelName) &&
                  sizeof(kScanKernels<true>) == sizeof(kScanKernels<false>),
              "kScanKernels: one row per row of kScanKernelNames (scan_plan.h), in its order");
constexpr bool scan_kernel_rows_match()
{
    for (int k = 0; k < static_cast<int>(ScanKernel::kNone); ++k)
        if (!kScanKernels<false>[k].fn || !kScanKernels<true>[k].fn == scan_kernel_decodes(static_cast<ScanKernel>(k), true)) return false;
    return true;
}
static_assert(scan_kernel_rows_match(), "kScanKernels: a row's decode fn is null exactly where scan_kernel_decodes (scan_plan.h) says the kernel serves no decode call at all");
const ScanKernelRow &row_of(ScanKernel k, bool decode = false) { return (decode ? kScanKernels<true> : kScanKernels<false>)[static_cast<int>(k)]; }

// BASIC_SCAN_KERNEL = generic | pipelined | batched | wavefront | band forces a kernel (identical results); anything else: kNone
ScanKernel forced_kernel()
{
    if (const char *e = getenv("BASIC_SCAN_KERNEL"))
        for (int k = 0; k < static_cast<int>(ScanKernel::kNone); ++k)
            if (!strcmp(e, kScanKernelNames[k].env)) return static_cast<ScanKernel>(k);
    return ScanKernel::kNone;
}

// grows the plan's scratch to `floats` and clears its granule regions
int ensure_scratch(basic_scanline_plan *p, size_t floats, size_t gran_floats, hipStream_t st)
{
    if (floats > p->scratch_cap) {
        if (p->d_scratch) (void)hipFree(p->d_scratch);
        p->d_scratch = nullptr; p->scratch_cap = 0;
        BASIC_HIP_TRY(hipMalloc(&p->d_scratch, floats * sizeof(float)));
        p->scratch_cap = floats;
    }
    BASIC_HIP_TRY(hipMemsetAsync(p->d_scratch, 0, gran_floats * sizeof(float), st));   // tag 0 = "not written in this launch"
    return BASIC_OK;
}

int device_cus(int *cus)
{
    int dev = 0;
    BASIC_HIP_TRY(hipGetDevice(&dev));
    BASIC_HIP_TRY(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev));
    return BASIC_OK;
}

// What the planner cannot know by itself: the device, the environment and the table set (`tables` != nullptr: decode; *tv: its fast
// search image, when it has one)
int make_request(const basic_rans_tables *tables, int batch, int h, int w, int table_len, int schedule, int lane_max_batch, ScanRequest *q,
                 RansFastView *tv)
{
    q->batch = batch; q->h = h; q->w = w; q->table_len = table_len;
    q->schedule = schedule; q->lane_max_batch = lane_max_batch;
    q->force = forced_kernel();
    q->decode = tables != nullptr;
    q->fast_image = q->decode && rans_fast_view(tables, tv) == BASIC_OK;
    q->decoder_lds = q->fast_image ? decoder_lds_bytes(tv->image_words, tv->rows) : 0;
    return device_cus(&q->cus);
}

// Plans a *_dev call: the plan's encode and decode schedules, no coder gates; `tables` != nullptr: decode
int prepare_launch(const basic_scanline_plan *p, int batch, int lanes, bool rows, int h, int w, int table_len, const basic_rans_tables *tables,
                   RansFastView *tv, ScanLaunch *L)
{
    ScanRequest q;
    const int rc = make_request(tables, batch, h, w, table_len, p->encode_schedule, -1, &q, tv);
    if (rc) return rc;
    q.lanes = lanes; q.rows = rows; q.decode_schedule = p->decode_schedule;
    if (tables && !q.fast_image) return rans_fast_view(tables, tv);   // no fast search image: its error
    return plan_scan(p, q, L);
}

// ---- launch arguments of one launch over `batch` images (of the call's `L.images` per launch)
// generic / pipelined kernels
int fill_args_lane(basic_scanline_plan *p, ScanArgs &a, const ScanLaunch &L, ScanScratch *sc, int batch, int h, int w, const float *d_prior, hipStream_t st)
{
    const int64_t HW = static_cast<int64_t>(h) * w;
    *sc = lane_scratch(p, batch, HW);
    int rc = ensure_scratch(p, sc->total, sc->gran_end, st);
    if (rc) return rc;
    for (int l = 0; l < p->nlayers; ++l) {
        a.rpw[l] = p->rpw[l]; a.woff[l] = p->woff[l];
        a.kgroup[l] = p->kgroup[l]; a.bpg[l] = p->bpg[l]; a.kpad[l] = p->kpad[l];
    }
    if (p->P > 0) {
        const int64_t total = static_cast<int64_t>(batch) * HW * p->P;
        int64_t g = (total + 255) / 256;
        hipLaunchKernelGGL(transpose_prior_kernel, dim3(static_cast<unsigned>(g > 4096 ? 4096 : g)), dim3(256), 0, st, d_prior, p->d_scratch + sc->prior, p->P,
                           static_cast<int>(HW), total);
        BASIC_HIP_TRY(hipGetLastError());
    }
    const ScanLaneLds &o = L.lane;
    a.tab_off = o.tab_off; a.ps_off = o.ps_off; a.xs_off = o.xs_off; a.part_off = o.part_off; a.flag_off = o.flag_off; a.bias_off = o.bias_off;
    a.x0_off = o.x0_off; a.early_off = o.early_off; a.desc_off = o.desc_off; a.bc = o.bc; a.part_floats = o.part_floats;
    return BASIC_OK;
}

// batched family (L.kernel: kBatched raster; kWavefront: yT [steps][C][yw], priorT [steps][P][nbt]; kBand: the band's)
int fill_args_batched(basic_scanline_plan *p, ScanArgs &a, const ScanLaunch &L, ScanScratch *sc, int batch, int h, int w, const float *d_prior, hipStream_t st)
{
    const bool wf = L.kernel != ScanKernel::kBatched, band = L.kernel == ScanKernel::kBand;
    const int pad = p->ksize / 2, yw = batch * (h + pad);
    const int64_t HW = wf ? wavefront_steps(p, h, w) : static_cast<int64_t>(h) * w;   // slabs of the coded latent and of the prior
    const int bA = band ? band_slots(p, w) : 0, ipt = band ? 32 / bA : 0;
    const int cols = batched_columns(p, L.kernel, batch, h, w);
    const int tiles = (cols + 31) / 32, nbt = 32 * tiles;
    if (wf) { a.wf_cols = cols; a.wf_s = wavefront_slope(p); a.wf_steps = static_cast<int>(HW); a.wf_yw = yw; }
    a.band_A = bA; a.band_ipt = ipt;
    a.nbt = nbt; a.nw = p->b_nw; a.nd = p->b_nd; a.bpt = p->b_bpt; a.ctx_blocks = p->b_ctx_blocks;
    *sc = batched_scratch(p, nbt, HW, yw, L.kernel);
    int rc = ensure_scratch(p, sc->total, sc->gran_end, st);
    if (rc) return rc;
    a.wlate = p->d_scratch + sc->wlate;
    for (int l = 0; l < p->nlayers; ++l) { a.nblk[l] = p->b_nblk[l]; a.rt[l] = p->b_rt[l]; a.tile_off[l] = p->b_tile_off[l]; }
    uint64_t *yT = reinterpret_cast<uint64_t *>(p->d_scratch + sc->yT);
    if (wf && pad > 0) {
        const int64_t total = HW * p->C * batch * pad;
        int64_t g = (total + 255) / 256;
        hipLaunchKernelGGL(wavefront_pads_kernel, dim3(static_cast<unsigned>(g > 8192 ? 8192 : g)), dim3(256), 0, st, yT, p->C, batch, h, pad, yw, total);
        BASIC_HIP_TRY(hipGetLastError());
    }
    if (band && pad > 0) {
        const int64_t total = static_cast<int64_t>(p->C) * batch * h * 2 * pad;
        int64_t g = (total + 255) / 256;
        hipLaunchKernelGGL(band_edges_kernel, dim3(static_cast<unsigned>(g > 8192 ? 8192 : g)), dim3(256), 0, st, yT, p->C, batch, h, w, a.wf_s, bA, pad,
                           a.wf_steps, yw, total);
        BASIC_HIP_TRY(hipGetLastError());
    }
    if (p->P > 0) {
        float *pT = p->d_scratch + sc->prior;
        const int64_t total = static_cast<int64_t>(cols) * HW * p->P;
        int64_t g = (total + 255) / 256;
        if (band)
            hipLaunchKernelGGL(transpose_prior_band_kernel, dim3(static_cast<unsigned>(g > 8192 ? 8192 : g)), dim3(256), 0, st, d_prior, pT, p->P, batch, h, w,
                               a.wf_s, bA, ipt, a.wf_steps, nbt, total);
        else if (wf)
            hipLaunchKernelGGL(transpose_prior_wavefront_kernel, dim3(static_cast<unsigned>(g > 8192 ? 8192 : g)), dim3(256), 0, st, d_prior, pT, p->P, h, w,
                               a.wf_s, a.wf_steps, nbt, total);
        else
            hipLaunchKernelGGL(transpose_prior_batched_kernel, dim3(static_cast<unsigned>(g > 8192 ? 8192 : g)), dim3(256), 0, st, d_prior, pT, batch,
                               p->P, static_cast<int>(HW), nbt, total);
        BASIC_HIP_TRY(hipGetLastError());
    }
    return BASIC_OK;
}

// The arguments of one launch of the call `L` plans, over `batch` of its images: the family's own, then what both families share.
// `first`: the first launch of the call, which also clears the barrier counter and the error flag (a later launch of the call
// keeps an earlier one's error flag).
int fill_args(basic_scanline_plan *p, ScanArgs &a, const ScanLaunch &L, int batch, int h, int w, const float *d_prior, const float *d_table, int table_len,
              bool first, hipStream_t st)
{
    const bool lane = L.kernel == ScanKernel::kGeneric || L.kernel == ScanKernel::kPipelined;
    ScanScratch sc;
    const int rc = lane ? fill_args_lane(p, a, L, &sc, batch, h, w, d_prior, st) : fill_args_batched(p, a, L, &sc, batch, h, w, d_prior, st);
    if (rc) return rc;
    a.B = batch; a.C = p->C; a.H = h; a.W = w; a.P = p->P;
    a.nlayers = p->nlayers; a.ntaps = p->ntaps; a.vec4 = p->vec4;
    a.table = d_table; a.table_len = table_len;
    const int nact = lane ? p->nlayers : p->nlayers - 1;
    for (int l = 0; l < p->nlayers; ++l) {
        a.rows[l] = p->rows[l]; a.kdim[l] = p->kdim[l]; a.act_after[l] = p->act_after[l];
        a.w[l] = p->d_w[l]; a.bias[l] = p->d_b[l];
        a.act[l] = l < nact ? reinterpret_cast<uint64_t *>(p->d_scratch + sc.act[l]) : nullptr;
    }
    a.yT = reinterpret_cast<uint64_t *>(p->d_scratch + sc.yT);
    a.mu = reinterpret_cast<uint64_t *>(p->d_scratch + sc.mu);
    a.idx_step = reinterpret_cast<uint64_t *>(p->d_scratch + sc.idx_step);
    a.priorT = p->P > 0 ? p->d_scratch + sc.prior : nullptr;
    // a tap's position relative to the coded one (wavefront, band: its slab relative to the step's: dx steps along the row, wf_s per row)
    const int row_stride = !lane && L.kernel != ScanKernel::kBatched ? wavefront_slope(p) : w;
    for (int t = 0; t < p->ntaps; ++t) { a.tap_dy[t] = p->tap_dy[t]; a.tap_dx[t] = p->tap_dx[t]; a.tap_off[t] = p->tap_dy[t] * row_stride + p->tap_dx[t]; }
    a.ncompute = compute_workgroups(p, L.kernel, batch, h, w);
    a.bar = p->d_bar;
    a.err = reinterpret_cast<int *>(p->d_bar + 1);
    if (first) BASIC_HIP_TRY(hipMemsetAsync(p->d_bar, 0, 2 * sizeof(unsigned), st));
    return BASIC_OK;
}

// BASIC_SCAN_PROFILE=1 (debugging aid): where does workgroup 0 spend a coding step?  Synchronises the stream.
struct ScanProfile {
    static constexpr int kSlots = 4 * kMaxLayers + 8;
    long long *d = nullptr;
    int begin(ScanArgs &a, hipStream_t st)
    {
        if (!getenv("BASIC_SCAN_PROFILE")) return BASIC_OK;
        BASIC_HIP_TRY(hipMalloc(&d, kSlots * sizeof(long long)));
        BASIC_HIP_TRY(hipMemsetAsync(d, 0, kSlots * sizeof(long long), st));
        a.prof = d;
        return BASIC_OK;
    }
    void report(const ScanArgs &a, hipStream_t st, const char *what)
    {
        if (!d) return;
        long long h[kSlots];
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
        (void)hipFree(d);
        d = nullptr;
        const double steps = a.wf_cols ? static_cast<double>(a.wf_steps) : static_cast<double>(a.H) * a.W;
        if (a.nbt) {   // batched kernel: first context workgroup (late: wave 1, early: wave 0), first dense workgroup (wave 0)
            fprintf(stderr, "scan-line %s profile, 10 ns ticks per coding step | context tile: wait for y %.1f, late block %.1f, barrier + finish %.1f, early half %.1f | ", what,
                    h[0] / steps, h[1] / steps, h[2] / steps, h[3] / steps);
            for (int l = 1; l < a.nlayers; ++l)
                fprintf(stderr, "dense L%d: prior blocks + wait %.1f, loads + chains %.1f, barrier + finish %.1f | ", l, h[4 * l] / steps, h[4 * l + 1] / steps, h[4 * l + 2] / steps);
        } else {
            fprintf(stderr, "scan-line %s profile (workgroup 0; 10 ns ticks per coding step: stage+wait / dots / finish / gauss): ", what);
            for (int l = 0; l < a.nlayers; ++l)
                fprintf(stderr, "L%d %.1f / %.1f / %.1f / %.1f | ", l, h[4 * l] / steps, h[4 * l + 1] / steps, h[4 * l + 2] / steps, h[4 * l + 3] / steps);
        }
        fprintf(stderr, "loop %.1f ticks per step, %.2f shader clocks per tick", h[4 * kMaxLayers + 1] / steps,
                h[4 * kMaxLayers + 1] ? static_cast<double>(h[4 * kMaxLayers]) / h[4 * kMaxLayers + 1] : 0.0);
        if (h[4 * kMaxLayers + 3])
            fprintf(stderr, " | decoder wave of stream 0: waiting %.1f, decoding %.1f (shader clocks per step: decode_chunk %.0f, publishing %.0f; stream words per step %.1f)", h[4 * kMaxLayers + 2] / steps,
                    h[4 * kMaxLayers + 3] / steps, h[4 * kMaxLayers + 4] / steps, h[4 * kMaxLayers + 5] / steps, h[4 * kMaxLayers + 6] / steps);
        fprintf(stderr, "\n");
    }
};

int run_launch(basic_scanline_plan *p, ScanArgs &a, const ScanLaunch &L, int grid, bool decode, hipStream_t st)
{
    const ScanKernelRow &k = row_of(L.kernel, decode);
    const ScanFn fn = k.fn;
    BASIC_REQUIRE(fn, "scanline: the kernel has no such form");
    BASIC_HIP_TRY(ensure_max_lds(reinterpret_cast<const void *>(fn)));
    ScanProfile prof;
    int rc = prof.begin(a, st);
    if (rc) return rc;
    p->last_kernel = scan_kernel_id(L.kernel);
    rc = chained_launch(p, st, grid, L.cus, [&] { hipLaunchKernelGGL(fn, dim3(grid), dim3(kThreads), L.lds_bytes, st, a); });
    prof.report(a, st, k.label);
    return rc;
}

// A whole *_dev call: plan it, then one launch after the other over whole images (one launch is the common case; the band takes
// more for a large batch): one stream, one scratch -- each launch clears and fills it in stream order.  `io`: the call's buffers,
// of which a launch gets those of its images.
int run_call(basic_scanline_plan *p, const ScanArgs &io, int batch, int h, int w, const float *d_prior, const float *d_table, int table_len,
             const basic_rans_tables *tables, hipStream_t st)
{
    ScanLaunch L;
    RansFastView tv;
    int rc = prepare_launch(p, batch, io.lanes, io.row_streams != 0, h, w, table_len, tables, &tv, &L);
    if (rc) return rc;
    const bool decode = tables != nullptr;
    const int64_t img_lat = static_cast<int64_t>(p->C) * h * w, img_prior = static_cast<int64_t>(p->P) * h * w;
    for (int b0 = 0; b0 < batch; b0 += L.images) {
        const int nb = std::min(L.images, batch - b0);
        ScanArgs a = io;
        if (decode) a.tv = tv;
        rc = fill_args(p, a, L, nb, h, w, d_prior ? d_prior + b0 * img_prior : nullptr, d_table, table_len, b0 == 0, st);
        if (rc) return rc;
        if (a.y) a.y += b0 * img_lat;
        a.ybuf += b0 * img_lat; a.sym += b0 * img_lat; a.idx += b0 * img_lat;
        // a launch after the first is the band's: a decode one reads its own images' row streams with its own decoder workgroups
        if (decode && b0 > 0) a.word_off += static_cast<int64_t>(b0) * h * io.lanes;
        const int short_grid = a.ncompute + (decode ? decoder_workgroups(nb * band_decode_slots(p, h, w) * io.lanes) : 0);
        rc = run_launch(p, a, L, nb == L.images ? L.grid : short_grid, decode, st);   // (a short last launch: the band's)
        if (rc) return rc;
    }
    return BASIC_OK;
}

}  // namespace

extern "C" int basic_scanline_encode_dev(basic_scanline_plan *p, const float *d_y, const float *d_prior, int batch, int h, int w,
                                         const float *d_table, int table_len, int32_t *d_symbols, int32_t *d_indexes, float *d_ybuf,
                                         void *hip_stream)
{
    BASIC_REQUIRE(p && d_y && d_table && d_symbols && d_indexes && d_ybuf && batch >= 1 && h >= 1 && w >= 1 && table_len >= 1 &&
                      table_len <= 4096 && (d_prior || p->P == 0),
                  "scanline_encode: bad argument");
    ScanArgs io{};
    io.y = d_y; io.ybuf = d_ybuf; io.sym = d_symbols; io.idx = d_indexes;
    io.lanes = 1; io.lane_w = p->C;
    return run_call(p, io, batch, h, w, d_prior, d_table, table_len, nullptr, as_stream(hip_stream));
}

namespace {

// a decode call over lane streams (rows == false: stream b * lanes + k) or row streams (stream (b * h + r) * lanes + k)
int decode_call(basic_scanline_plan *p, const basic_rans_tables *tables, const uint32_t *d_words, const int64_t *d_word_off, const float *d_prior,
                int batch, int lanes, bool rows, int h, int w, const float *d_table, int table_len, int32_t *d_symbols, int32_t *d_indexes,
                float *d_ybuf, void *hip_stream)
{
    BASIC_REQUIRE(p && tables && d_words && d_word_off && d_table && d_symbols && d_indexes && d_ybuf && batch >= 1 && h >= 1 && w >= 1 &&
                      table_len >= 1 && table_len <= 4096 && (d_prior || p->P == 0),
                  "scanline_decode: bad argument");
    BASIC_REQUIRE(valid_lanes(p, lanes) && static_cast<int64_t>(batch) * lanes * (rows ? h : 1) < (1ll << 30),
                  "scanline_decode: lanes must divide the channels into runs of a multiple of 16");
    ScanArgs io{};
    io.ybuf = d_ybuf; io.sym = d_symbols; io.idx = d_indexes; io.words = d_words; io.word_off = d_word_off;
    io.lanes = lanes; io.lane_w = p->C / lanes; io.row_streams = rows ? 1 : 0;
    return run_call(p, io, batch, h, w, d_prior, d_table, table_len, tables, as_stream(hip_stream));
}

}  // namespace

extern "C" int basic_scanline_decode_lanes_dev(basic_scanline_plan *p, const basic_rans_tables *tables, const uint32_t *d_words,
                                               const int64_t *d_word_off, const float *d_prior, int batch, int lanes, int h, int w,
                                               const float *d_table, int table_len, int32_t *d_symbols, int32_t *d_indexes, float *d_ybuf,
                                               void *hip_stream)
{
    return decode_call(p, tables, d_words, d_word_off, d_prior, batch, lanes, false, h, w, d_table, table_len, d_symbols, d_indexes, d_ybuf, hip_stream);
}

// basic_scanline_decode_lanes_dev for ROW STREAMS: batch * h * lanes streams, stream (b * h + r) * lanes + k carries row r of image
// b, lane k.  Where the call fits (wavefront_decode_fits) and the rule, the plan's decode schedule or BASIC_SCAN_KERNEL=wavefront says
// so, the wavefront decode launch; under the band decode schedule or BASIC_SCAN_KERNEL=band the band decode launch(es); otherwise the
// raster kernels, whose decoder wavefronts change stream at every row start.
extern "C" int basic_scanline_decode_rows_dev(basic_scanline_plan *p, const basic_rans_tables *tables, const uint32_t *d_words,
                                              const int64_t *d_word_off, const float *d_prior, int batch, int lanes, int h, int w,
                                              const float *d_table, int table_len, int32_t *d_symbols, int32_t *d_indexes, float *d_ybuf,
                                              void *hip_stream)
{
    return decode_call(p, tables, d_words, d_word_off, d_prior, batch, lanes, true, h, w, d_table, table_len, d_symbols, d_indexes, d_ybuf, hip_stream);
}

extern "C" int basic_scanline_decode_dev(basic_scanline_plan *p, const basic_rans_tables *tables, const uint32_t *d_words,
                                         const int64_t *d_word_off, const float *d_prior, int batch, int h, int w, const float *d_table,
                                         int table_len, int32_t *d_symbols, int32_t *d_indexes, float *d_ybuf, void *hip_stream)
{
    return basic_scanline_decode_lanes_dev(p, tables, d_words, d_word_off, d_prior, batch, 1, h, w, d_table, table_len, d_symbols, d_indexes,
                                           d_ybuf, hip_stream);
}

// What a basic_scanline_encode_dev (tables == nullptr) or basic_scanline_decode_lanes_dev call (basic_scanline_decode_dev: lanes = 1)
// with these arguments would run -- a decode call's decoder workgroups are those of its batch * lanes streams (the wavefront decode
// launch of a row-stream call: batch * h * lanes) --, after the
// coder's gates (ScanRequest::lane_max_batch): *kernel = BASIC_SCAN_KERNEL_NONE leaves the call to the per-step path, which codes
// the same integers.  Launches nothing.
// (rows != 0: a decode call over row streams, basic_scanline_decode_rows_dev; encode calls do not depend on it)
extern "C" int basic_scanline_choose_rows(const basic_scanline_plan *p, const basic_rans_tables *tables, int batch, int lanes, int rows, int h,
                                          int w, int table_len, int schedule, int lane_max_batch, int *kernel, int *launches)
{
    BASIC_REQUIRE(p && kernel && batch >= 1 && h >= 0 && w >= 0 && table_len >= 1 && table_len <= 4096 && lane_max_batch >= 0 &&
                      schedule >= BASIC_SCAN_SCHEDULE_AUTO && schedule <= BASIC_SCAN_SCHEDULE_BAND,
                  "scanline_choose: bad argument");
    BASIC_REQUIRE(valid_lanes(p, lanes) && static_cast<int64_t>(batch) * lanes * (rows && h > 0 ? h : 1) < (1ll << 30),
                  "scanline_choose: lanes must divide the channels into runs of a multiple of 16");
    ScanRequest q;
    RansFastView tv;
    ScanLaunch L;
    int rc = make_request(tables, batch, h, w, table_len, schedule, lane_max_batch, &q, &tv);
    if (rc) return rc;
    q.lanes = lanes; q.rows = rows != 0 && tables != nullptr; q.decode_schedule = p->decode_schedule;
    rc = plan_scan(p, q, &L);
    if (rc) return rc;
    *kernel = L.kernel == ScanKernel::kNone ? BASIC_SCAN_KERNEL_NONE : scan_kernel_id(L.kernel);
    if (launches) *launches = L.launches;
    return BASIC_OK;
}

extern "C" int basic_scanline_choose_lanes(const basic_scanline_plan *p, const basic_rans_tables *tables, int batch, int lanes, int h, int w,
                                           int table_len, int schedule, int lane_max_batch, int *kernel, int *launches)
{
    return basic_scanline_choose_rows(p, tables, batch, lanes, 0, h, w, table_len, schedule, lane_max_batch, kernel, launches);
}

extern "C" int basic_scanline_choose(const basic_scanline_plan *p, const basic_rans_tables *tables, int batch, int h, int w, int table_len,
                                     int schedule, int lane_max_batch, int *kernel, int *launches)
{
    return basic_scanline_choose_lanes(p, tables, batch, 1, h, w, table_len, schedule, lane_max_batch, kernel, launches);
}

// Whether basic_scanline_decode_dev can serve `batch` streams of this table set on the current device (the set has a fast
// search image that fits the LDS, and compute + decoder workgroups fit the chip).  Both paths code the same integers, so a
// caller that gets 0 simply decodes with the per-step path.
extern "C" int basic_scanline_can_decode(const basic_scanline_plan *p, const basic_rans_tables *tables, int batch, int *ok)
{
    BASIC_REQUIRE(p && tables && ok && batch >= 1, "scanline_can_decode: bad argument");
    *ok = 0;
    RansFastView tv;
    if (rans_fast_view(tables, &tv) != BASIC_OK) return BASIC_OK;
    int cus = 0;
    int rc = device_cus(&cus);
    if (rc) return rc;
    *ok = lane_grid_resident(p, decoder_workgroups(batch), cus) && decoder_lds_bytes(tv.image_words, tv.rows) <= kMaxLds;
    return BASIC_OK;
}

// The largest batch the batched kernel (the batch as the N dimension of MFMA tiles, weights in registers) serves for a latent
// `w` columns wide on the current device: 0 = never (the layers do not have its shape, or the latent is too narrow);
// `decode` != 0 counts the decoder workgroups (one wavefront per image stream) too.
extern "C" int basic_scanline_batched_max(const basic_scanline_plan *p, int w, int decode, int *max_batch)
{
    BASIC_REQUIRE(p && max_batch && w >= 1, "scanline_batched_max: bad argument");
    *max_batch = 0;
    int cus = 0;
    int rc = device_cus(&cus);
    if (rc) return rc;
    *max_batch = batched_max_batch(p, w, decode != 0, cus);
    return BASIC_OK;
}

// The largest batch the wavefront encode schedule serves for an h x w latent on the current device: 0 = never (the layers do
// not have the batched kernel's shape, h alone needs more than its 64 columns, or the grid is not resident).  Any width fits.
extern "C" int basic_scanline_wavefront_max(const basic_scanline_plan *p, int h, int w, int *max_batch)
{
    BASIC_REQUIRE(p && max_batch && h >= 1 && w >= 1, "scanline_wavefront_max: bad argument");
    *max_batch = 0;
    int cus = 0;
    int rc = device_cus(&cus);
    if (rc) return rc;
    *max_batch = wavefront_max_batch(p, h, cus);
    return BASIC_OK;
}

// The images ONE launch of the band encode schedule codes of an h x w latent on the current device; a larger batch takes several
// launches inside one call.  0 = never: the layers do not have the batched kernel's shape, the latent is so wide that an image's
// slots (w / (ksize / 2 + 2) + 1) exceed one 32-column tile, or a single image is too large for the scratch limit or for the
// kernel's 32-bit offsets.
extern "C" int basic_scanline_band_max(const basic_scanline_plan *p, int h, int w, int *images_per_launch)
{
    BASIC_REQUIRE(p && images_per_launch && h >= 1 && w >= 1, "scanline_band_max: bad argument");
    *images_per_launch = 0;
    int cus = 0;
    int rc = device_cus(&cus);
    if (rc) return rc;
    *images_per_launch = band_images_per_launch(p, h, w, cus);
    return BASIC_OK;
}

// The images ONE launch of the band decode launch (row streams) decodes of an h x w latent in `lanes` lane streams on the current
// device: the largest number whose column tiles' workgroups and decoder workgroups -- one wavefront per (image, slot, lane), four to
// a workgroup -- fit the chip together; a larger batch takes several launches inside one call.  0 = never: what
// basic_scanline_band_max says, no room for an image's decoder wavefronts beside its tile, or a table set without a fast search
// image that fits the LDS.
extern "C" int basic_scanline_band_decode_max(const basic_scanline_plan *p, const basic_rans_tables *tables, int h, int w, int lanes,
                                              int *images_per_launch)
{
    BASIC_REQUIRE(p && tables && images_per_launch && h >= 1 && w >= 1, "scanline_band_decode_max: bad argument");
    BASIC_REQUIRE(valid_lanes(p, lanes), "scanline_band_decode_max: lanes must divide the channels into runs of a multiple of 16");
    *images_per_launch = 0;
    RansFastView tv;
    if (rans_fast_view(tables, &tv) != BASIC_OK || decoder_lds_bytes(tv.image_words, tv.rows) > kMaxLds) return BASIC_OK;
    int cus = 0;
    int rc = device_cus(&cus);
    if (rc) return rc;
    *images_per_launch = band_decode_images_per_launch(p, h, w, lanes, cus);
    return BASIC_OK;
}

// Which kernel the plan's last launch (either direction) ran: BASIC_SCAN_KERNEL_*; NONE before the first launch.
extern "C" int basic_scanline_last_kernel(const basic_scanline_plan *p, int *kernel)
{
    BASIC_REQUIRE(p && kernel, "scanline_last_kernel: bad argument");
    *kernel = p->last_kernel;
    return BASIC_OK;
}

extern "C" int basic_scanline_set_encode_schedule(basic_scanline_plan *p, int schedule)
{
    BASIC_REQUIRE(p && (schedule == BASIC_SCAN_SCHEDULE_AUTO || schedule == BASIC_SCAN_SCHEDULE_RASTER || schedule == BASIC_SCAN_SCHEDULE_WAVEFRONT ||
                       schedule == BASIC_SCAN_SCHEDULE_BAND),
                  "scanline_set_encode_schedule: bad argument");
    p->encode_schedule = schedule;
    return BASIC_OK;
}

// The schedule of the plan's row-stream decode calls (basic_scanline_decode_rows_dev; basic_scanline_choose_rows with rows != 0
// answers for it): BASIC_SCAN_SCHEDULE_*, as for encode.  Calls without row streams never look at it.
extern "C" int basic_scanline_set_decode_schedule(basic_scanline_plan *p, int schedule)
{
    BASIC_REQUIRE(p && (schedule == BASIC_SCAN_SCHEDULE_AUTO || schedule == BASIC_SCAN_SCHEDULE_RASTER || schedule == BASIC_SCAN_SCHEDULE_WAVEFRONT ||
                       schedule == BASIC_SCAN_SCHEDULE_BAND),
                  "scanline_set_decode_schedule: bad argument");
    p->decode_schedule = schedule;
    return BASIC_OK;
}

// 0 = the last launch on this plan completed its barriers; 1 = a barrier timed out (results invalid).  Synchronises `hip_stream`.
extern "C" int basic_scanline_status(basic_scanline_plan *p, void *hip_stream, int *poisoned)
{
    BASIC_REQUIRE(p && poisoned, "scanline_status: bad argument");
    unsigned h[2] = {0, 0};
    BASIC_HIP_TRY(hipMemcpyAsync(h, p->d_bar, sizeof(h), hipMemcpyDeviceToHost, as_stream(hip_stream)));
    BASIC_HIP_TRY(hipStreamSynchronize(as_stream(hip_stream)));
    *poisoned = h[1] != 0;
    return BASIC_OK;
}