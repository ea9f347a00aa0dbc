// The host-only planner of the persistent scan-line coder (scanline.hip): the constants it shares with the kernels, the integer
// geometry of a plan (scan_geometry: taps, canonical blocks, workgroups, weight offsets, the batched kernel's shape test), the
// scratch and LDS layouts, and plan_scan, the one place that decides how a scan-line call runs -- which kernel, in how many
// launches, with which grid and LDS.  Every rule here counts workgroups against compute units, bytes against LDS or element
// offsets against 2^31, and the spin-waiting grids of scanline.hip rest on them, so this header needs no HIP and no device: it
// includes standard headers and the C ABI only, reads no environment, dereferences no device pointer, and compiles under hipcc
// (scanline.hip includes it) and under a plain host compiler.  scan_plan_check.cpp replays recorded calls through it and sweeps
// its invariants on the CPU (tests/test_cpu_scan_plan.py; make scan_plan_check, SAN=1 for the sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "common_host.h"

namespace basic {

constexpr int kThreads = 256;
constexpr int kMaxLayers = 5;   // context convolution + up to four dense layers
constexpr int kMaxTaps = 24;    // causal taps of a k x k window: (k/2) * k + k/2  (k = 7 -> 24)
constexpr int kKB = BASIC_MCONV_BLOCK_CHANNELS;
constexpr int kBlockPad = 4;   // LDS floats between the blocks of a weight row: lanes working on different blocks of a row start on different banks
constexpr int kWinU = 6;   // early-window granule pairs per thread: (ntaps - 1) * C / 2 <= 6 * 256 per image
constexpr int kBSlots = 8;        // weight blocks a wave keeps in registers for the whole launch (256 registers: the accumulator half of the file)
constexpr int kBLate = 4;         // context role: the LAST four blocks of the K axis (the left neighbour's among them) run in the late half, one per
                                  // wave, with weights re-fetched every step from the workgroup's fragment copy (a ninth resident block spills)
constexpr int kBDenseSlots = 3;   // blocks per dense layer and wave (a layer's K axis has at most 12; the last layer's at most 8: slots 6, 7)
constexpr int kBTile = 1024;      // floats of a 32 x 32 partial tile

// ---- The integer geometry of a plan: everything basic_scanline_plan knows that is not device state
struct ScanGeometry {
    int C = 0, P = 0, ksize = 0, nlayers = 0, ntaps = 0, nwg = 1, vec4 = 0;
    int rows[kMaxLayers] = {}, kdim[kMaxLayers] = {}, rpw[kMaxLayers] = {}, woff[kMaxLayers] = {}, act_after[kMaxLayers] = {};
    int kgroup[kMaxLayers] = {}, bpg[kMaxLayers] = {}, kpad[kMaxLayers] = {};   // canonical blocks (see scanline.hip's header comment)
    int tap_dy[kMaxTaps] = {}, tap_dx[kMaxTaps] = {};
    int weight_floats = 0;   // LDS floats of one workgroup's weight slices
    // batched kernel (scanline_batched_kernel): whether the layers have its shape, and the split of a column tile's workgroups
    bool batched = false;
    int b_nw = 0, b_nd = 0, b_bpt = 0, b_ctx_blocks = 0;
    int b_nblk[kMaxLayers] = {}, b_rt[kMaxLayers] = {}, b_tile_off[kMaxLayers] = {};
    int b_tiles = 0;             // partial tiles (4 KB each) the larger role keeps in LDS
};

// The arithmetic half of basic_scanline_plan_create: the taps, K groups, canonical blocks, the workgroup search, the weight offsets
// and the batched-kernel shape test.  Allocates nothing; refuses what plan_create refuses.
inline int scan_geometry(int channels, int ctx_out, int ksize, int prior_channels, int n_dense, const int *dense_out, const int *act_after,
                         const int *dense_in_groups, ScanGeometry *p)
{
    BASIC_REQUIRE(p && channels >= 1 && ctx_out >= 2 && (ksize == 3 || ksize == 5 || ksize == 7) && n_dense >= 1 && n_dense <= kMaxLayers - 1 &&
                      dense_out && act_after && prior_channels >= 0,
                  "scanline_plan_create: bad argument");
    BASIC_REQUIRE(dense_out[n_dense - 1] == 2 * channels, "scanline_plan_create: the last layer must give (mean, scale) pairs: 2 * channels rows");
    *p = ScanGeometry{};
    p->C = channels; p->P = prior_channels; p->ksize = ksize; p->nlayers = 1 + n_dense;
    const int half = ksize / 2;
    for (int ky = 0; ky <= half; ++ky)
        for (int kx = 0; kx < ksize; ++kx) {
            if (ky == half && kx >= half) break;
            p->tap_dy[p->ntaps] = ky - half; p->tap_dx[p->ntaps] = kx - half;
            ++p->ntaps;
        }
    p->rows[0] = ctx_out; p->kdim[0] = p->ntaps * channels; p->act_after[0] = act_after[0];
    for (int l = 1; l <= n_dense; ++l) {
        p->rows[l] = dense_out[l - 1];
        p->kdim[l] = p->rows[l - 1] + (l == 1 ? prior_channels : 0);
        p->act_after[l] = act_after[l];
    }
    // canonical blocks: the context layer's K groups are its taps; a dense layer's are its in_groups equal channel groups
    // (the channel groups of the masked convolution it stands for: cat(ctx, prior) of the first merger layer is two)
    p->kgroup[0] = channels;
    for (int l = 1; l <= n_dense; ++l) {
        const int gi = dense_in_groups ? dense_in_groups[l - 1] : 1;
        BASIC_REQUIRE(gi >= 1 && p->kdim[l] % gi == 0, "scanline_plan_create: a dense layer's inputs do not divide into its channel groups");
        p->kgroup[l] = p->kdim[l] / gi;
    }
    p->vec4 = channels % 4 == 0 && prior_channels % 4 == 0;
    for (int l = 0; l < p->nlayers; ++l) p->vec4 = p->vec4 && p->rows[l] % 4 == 0 && p->kdim[l] % 4 == 0 && p->kgroup[l] % 4 == 0;
    for (int l = 0; l < p->nlayers; ++l) {
        p->bpg[l] = (p->kgroup[l] + kKB - 1) / kKB;
        // row = its groups' channels + kBlockPad floats after every block, + one more pad so that consecutive rows shift banks
        p->kpad[l] = (p->kdim[l] / p->kgroup[l]) * (p->kgroup[l] + kBlockPad * p->bpg[l]) + (p->vec4 ? 4 : 1);
    }
    // workgroups: the fewest (<= 192: the decoder adds its own) whose weight slices fit ~126 KB of LDS (BaSIC, C = 192: 64 --
    // three launches of concurrent stream workers then hold 195 of the 256 compute units and leave the rest to the transforms;
    // with 112 KB it was 77 and the workers' transforms queued behind the persistent launches); every layer in whole rows per workgroup, the
    // last one in whole (mean, scale) pairs
    constexpr size_t kWeightKB = 126;
    int nwg = 1;
    for (;; ++nwg) {
        int floats = 0;
        for (int l = 0; l < p->nlayers; ++l) {
            int rpw = (p->rows[l] + nwg - 1) / nwg;
            if (l == p->nlayers - 1) rpw = (rpw + 1) & ~1;
            floats += rpw * p->kpad[l];
        }
        if (floats * sizeof(float) <= kWeightKB * 1024 || nwg >= 192) { p->weight_floats = floats; break; }
    }
    BASIC_REQUIRE(p->weight_floats * sizeof(float) <= 150 * 1024, "scanline_plan_create: the layers do not fit the LDS of 192 compute units");
    p->nwg = nwg;
    int off = 0;
    for (int l = 0; l < p->nlayers; ++l) {
        int rpw = (p->rows[l] + nwg - 1) / nwg;
        if (l == p->nlayers - 1) rpw = (rpw + 1) & ~1;
        p->rpw[l] = rpw;
        p->woff[l] = off;
        off += (rpw * p->kpad[l] + 3) & ~3;
    }
    p->weight_floats = off;
    // batched kernel: every layer in whole 32-row tiles and whole 64-channel canonical blocks (no short block, none across a
    // K group or the ctx | prior seam); a context row tile's blocks in the nine register slots of four waves (the late blocks
    // on waves 1 .. bpt, slot 8); at most three blocks per dense layer and wave; at most three dense layers
    {
        bool ok = p->nlayers >= 2 && p->nlayers <= 4 && channels % kKB == 0 && channels / kKB <= kBLate - 1 && p->rows[0] % kKB == 0;
        const int bpt = channels / kKB, nb0 = p->ntaps * bpt;
        ok = ok && nb0 >= kBLate && nb0 - kBLate <= 4 * kBSlots;   // four late blocks (all of the left neighbour's among them), 8 resident per wave
        for (int l = 0; l < p->nlayers && ok; ++l) {
            ok = p->rows[l] % 32 == 0 && p->kdim[l] % kKB == 0 && p->kgroup[l] % kKB == 0;
            p->b_nblk[l] = p->kdim[l] / kKB;
            p->b_rt[l] = p->rows[l] / 32;
            if (l > 0) ok = ok && p->b_nblk[l] <= 4 * (l < 3 ? kBDenseSlots : kBSlots - 2 * kBDenseSlots);   // register slots 0-2, 3-5, 6-7
        }
        if (ok) {
            p->b_bpt = bpt;
            p->b_ctx_blocks = p->rows[0] / kKB;
            int tiles = 0;
            for (int l = 1; l < p->nlayers; ++l) {
                p->b_nd = std::max(p->b_nd, p->b_rt[l]);
                p->b_tile_off[l] = tiles * kBTile;
                tiles += p->b_nblk[l];
            }
            p->b_nw = p->b_nd + p->b_rt[0];
            p->b_tiles = std::max(tiles, p->b_nblk[0]);
            ok = static_cast<size_t>(p->b_tiles) * kBTile * sizeof(float) + 8192 <= 160 * 1024;
        }
        p->batched = ok;
    }
    return BASIC_OK;
}

inline size_t align4(size_t n) { return (n + 3) & ~static_cast<size_t>(3); }

// ---- The persistent kernels: the one list of them, in the order the planner considers them; a row's index is its ScanKernel.
enum class ScanKernel { kBand, kWavefront, kBatched, kPipelined, kGeneric, kNone };
// Their BASIC_SCAN_KERNEL_* ids (what basic_scanline_last_kernel and basic_scanline_choose report) and their spellings in the
// BASIC_SCAN_KERNEL environment variable; scanline.hip's kScanKernels adds what needs HIP, the labels and the function pointers.
struct ScanKernelName { int id; const char *env; };
constexpr ScanKernelName kScanKernelNames[] = {
    {BASIC_SCAN_KERNEL_BAND, "band"},           {BASIC_SCAN_KERNEL_WAVEFRONT, "wavefront"}, {BASIC_SCAN_KERNEL_BATCHED, "batched"},
    {BASIC_SCAN_KERNEL_PIPELINED, "pipelined"}, {BASIC_SCAN_KERNEL_GENERIC, "generic"},
};
constexpr int scan_kernel_id(ScanKernel k) { return kScanKernelNames[static_cast<int>(k)].id; }
static_assert(sizeof(kScanKernelNames) / sizeof(ScanKernelName) == static_cast<int>(ScanKernel::kNone) &&
                  scan_kernel_id(ScanKernel::kBand) == BASIC_SCAN_KERNEL_BAND && scan_kernel_id(ScanKernel::kWavefront) == BASIC_SCAN_KERNEL_WAVEFRONT &&
                  scan_kernel_id(ScanKernel::kBatched) == BASIC_SCAN_KERNEL_BATCHED && scan_kernel_id(ScanKernel::kPipelined) == BASIC_SCAN_KERNEL_PIPELINED &&
                  scan_kernel_id(ScanKernel::kGeneric) == BASIC_SCAN_KERNEL_GENERIC,
              "kScanKernelNames: one row per ScanKernel, in its order, with the id include/basic_hip.h gives it");
// whether the kernel serves a decode call: the raster kernels always, the wavefront and the band only a call that brings row streams
constexpr bool scan_kernel_decodes(ScanKernel k, bool rows) { return rows || (k != ScanKernel::kBand && k != ScanKernel::kWavefront); }

constexpr size_t kMaxLds = 160 * 1024;
// more than half of a compute unit's LDS per workgroup: exactly one workgroup per unit, as the barrier protocol assumes
constexpr size_t kMinLds = 96 * 1024;

// ---- The scratch of a launch, in floats from basic_scanline_plan::d_scratch:
// [granule regions: layer exchange arrays, coded latent, step means / rows][position-major prior][late fragments]
struct ScanScratch {
    size_t act[kMaxLayers] = {};            // layer exchange arrays (the first `nact` layers)
    size_t yT = 0, mu = 0, idx_step = 0;    // coded latent, step means, step rows
    size_t gran_end = 0;                    // the granule regions end here: cleared before every launch (tag 0 = "not written in this launch")
    size_t prior = 0, wlate = 0, total = 0;
};

// `cols` columns (images, or MFMA columns) of exchange / step / prior data, a coded latent of `ycols` columns, both in `slabs` steps
inline ScanScratch scratch_layout(const ScanGeometry *p, int nact, size_t cols, size_t ycols, int64_t slabs, size_t late_floats)
{
    ScanScratch s;
    size_t floats = 0;
    for (int l = 0; l < nact; ++l) { s.act[l] = floats; floats += align4(2 * cols * p->rows[l]); }
    s.yT = floats;       floats += align4(2 * ycols * slabs * p->C);
    s.mu = floats;       floats += align4(2 * cols * p->C);
    s.idx_step = floats; floats += align4(2 * cols * p->C);
    s.gran_end = floats;
    s.prior = floats;    floats += align4(cols * slabs * p->P);
    s.wlate = floats;    floats += late_floats;
    s.total = floats;
    return s;
}

// lane kernels (generic / pipelined): every layer exchanges [batch][rows], coded latent [HW][batch][C], prior [batch][HW][P]
inline ScanScratch lane_scratch(const ScanGeometry *p, int batch, int64_t hw) { return scratch_layout(p, p->nlayers, batch, batch, hw, 0); }

// batched family: exchange arrays [rows][nbt] of all layers but the last, coded latent [slabs][C][nbt] (raster) or [slabs][C][yw]
// (wavefront, band), step means / rows [nbt][C], prior [slabs][P][nbt], late fragments per workgroup
inline ScanScratch batched_scratch(const ScanGeometry *p, int nbt, int64_t slabs, int yw, ScanKernel mode)
{
    return scratch_layout(p, p->nlayers - 1, nbt, mode == ScanKernel::kBatched ? nbt : yw, slabs, static_cast<size_t>(nbt / 32) * p->b_nw * kThreads * 32);
}

// ---- LDS of a compute workgroup of the lane kernels, and which of the two serves the call
struct ScanLaneLds {
    int tab_off = 0, ps_off = 0, xs_off = 0, part_off = 0, flag_off = 0, bias_off = 0, x0_off = 0, early_off = 0, desc_off = 0;
    int bc = 0, part_floats = 0;
    bool pipelined = false;
    size_t lds_bytes = 0;
};

// The pipelined kernel is taken when it fits, unless `force` names the generic one.
inline int lane_lds(const ScanGeometry *p, int batch, int w, int table_len, ScanKernel force, ScanLaneLds *o)
{
    int kmax = 0;
    for (int l = 0; l < p->nlayers; ++l) kmax = p->kdim[l] > kmax ? p->kdim[l] : kmax;
    // LDS: [weights][table][params of a chunk][inputs of a chunk][flag]; as many images per chunk as fit (at most 8)
    const int total_floats = kMaxLds / 4 - 16;
    o->tab_off = static_cast<int>(align4(p->weight_floats));
    o->ps_off = o->tab_off + static_cast<int>(align4(table_len));
    const int rpw_last = p->rpw[p->nlayers - 1];
    int bc = 8 < batch ? 8 : batch;
    // one round of block partials: [blocks][items]; 1024 floats hold a batch-1 layer in one round (<= 36 blocks x ~10 rows)
    o->part_floats = 1024;
    for (int l = 0; l < p->nlayers; ++l)
        BASIC_REQUIRE((p->kdim[l] / p->kgroup[l]) * p->bpg[l] <= o->part_floats, "scanline: too many summation blocks in a layer");
    int bias_need = 0;
    for (int l = 0; l < p->nlayers; ++l) bias_need += p->rpw[l];
    auto need = [&](int n) { return o->ps_off + static_cast<int>(align4(n * rpw_last)) + static_cast<int>(align4(n * kmax)) + o->part_floats + 4 + static_cast<int>(align4(bias_need)); };
    while (bc > 1 && need(bc) > total_floats) --bc;
    BASIC_REQUIRE(need(bc) <= total_floats, "scanline: layer inputs do not fit the LDS");
    o->bc = bc;
    o->xs_off = o->ps_off + static_cast<int>(align4(bc * rpw_last));
    o->part_off = o->xs_off + static_cast<int>(align4(bc * kmax));
    o->flag_off = o->part_off + o->part_floats;
    o->bias_off = o->flag_off + 4;
    o->lds_bytes = static_cast<size_t>(o->bias_off + static_cast<int>(align4(bias_need))) * sizeof(float);
    // pipelined kernel: [weights][table][biases][context window B x K0][dense inputs B x Kd][partials][early sums][unit descriptors][flag]
    // -- taken when all of it fits (results are identical either way)
    int kd = 0, units_total = 0, units_max = 0;
    for (int l = 0; l < p->nlayers; ++l) {
        if (l > 0) kd = p->kdim[l] > kd ? p->kdim[l] : kd;
        const int u = batch * p->rpw[l] * (p->kdim[l] / p->kgroup[l]) * p->bpg[l];
        units_total += u;
        units_max = u > units_max ? u : units_max;
    }
    const size_t bias_off = align4(static_cast<size_t>(o->tab_off) + table_len);
    const size_t x0_off = bias_off + align4(bias_need);
    const size_t xs_off = x0_off + align4(static_cast<size_t>(batch) * p->kdim[0]);
    const size_t part_off = xs_off + align4(static_cast<size_t>(batch) * kd);
    const size_t early_off = part_off + align4(units_max);
    const size_t desc_off = early_off + align4(static_cast<size_t>(batch) * p->rpw[0]) +
                            align4(static_cast<size_t>(batch) * p->rpw[0] * (p->kdim[0] / p->kgroup[0]) * p->bpg[0]);   // early sums + the early blocks' partials
    const size_t flag_off = desc_off + align4(2 * static_cast<size_t>(units_total));
    // (the early half of a position's context window must be coded two steps before it: the tap up and to the right by
    // ksize / 2 columns is w - ksize / 2 positions back, so the latent must be at least ksize / 2 + 2 columns wide)
    bool fits = flag_off + 4 <= static_cast<size_t>(total_floats) && p->vec4 && (p->ntaps - 1) * (p->C / 2) <= kWinU * kThreads &&
                w >= p->ksize / 2 + 2;
    for (int l = 0; l < p->nlayers; ++l) fits = fits && batch * p->rpw[l] <= kThreads;   // one finishing item per thread
    if (force == ScanKernel::kGeneric) fits = false;
    if (force == ScanKernel::kPipelined) BASIC_REQUIRE(fits, "scanline: BASIC_SCAN_KERNEL=pipelined, but this batch does not fit the LDS");
    o->pipelined = fits;
    if (fits) {
        o->bias_off = static_cast<int>(bias_off); o->x0_off = static_cast<int>(x0_off); o->xs_off = static_cast<int>(xs_off);
        o->part_off = static_cast<int>(part_off); o->early_off = static_cast<int>(early_off); o->desc_off = static_cast<int>(desc_off);
        o->flag_off = static_cast<int>(flag_off);
        o->bc = batch;
        o->lds_bytes = (flag_off + 4) * sizeof(float);
    }
    return BASIC_OK;
}

// ---- batched kernel: when it serves a call
constexpr int kBatchedMaxTiles = 2;   // column tiles of 32 images per launch

// decoder workgroups of `streams` streams (one wavefront per stream; a decode call has batch * lanes of them)
inline int decoder_workgroups(int streams) { return (streams + kThreads / 64 - 1) / (kThreads / 64); }

// LDS of a decoder workgroup: the fast search image of the table set
inline size_t decoder_lds_bytes(int image_words, int rows)
{
    return (static_cast<size_t>((image_words + 3) & ~3) + 4 * static_cast<size_t>(rows) + 4) * sizeof(uint32_t);
}

// whether the batched kernel can serve `batch` images of a latent `w` columns wide (the context window's early half must be coded
// two steps before it is used: w >= ksize / 2 + 2); grid = column tiles x workgroups per tile (+ decoder workgroups)
inline bool batched_fits(const ScanGeometry *p, int batch, int w, int ndec, int cus)
{
    if (!p->batched || batch < 1 || batch > 32 * kBatchedMaxTiles || w < p->ksize / 2 + 2) return false;
    const int tiles = (batch + 31) / 32;
    return tiles * p->b_nw + ndec <= cus;
}

// basic_scanline_batched_max: the largest whole number of column tiles that fits, in images
inline int batched_max_batch(const ScanGeometry *p, int w, bool decode, int cus, int lanes = 1)
{
    for (int b = 32 * kBatchedMaxTiles; b >= 1; b -= 32)
        if (batched_fits(p, b, w, decode ? decoder_workgroups(b * lanes) : 0, cus)) return b;
    return 0;
}

// ---- wavefront encode schedule of the batched kernel: a column is one row of one image, so batch * h columns in at most
// kBatchedMaxTiles tiles; a row starts ksize / 2 + 2 steps after the row above it, which leaves the left neighbour as the only
// tap coded one step ago (the late half), every other one at least two (the early half).  No lower bound on the width: the
// zero padding left and right of a row is what its idle column publishes.
inline int wavefront_slope(const ScanGeometry *p) { return p->ksize / 2 + 2; }
inline int64_t wavefront_steps(const ScanGeometry *p, int h, int w) { return w + static_cast<int64_t>(wavefront_slope(p)) * (h - 1); }

inline bool wavefront_fits(const ScanGeometry *p, int batch, int h, int cus)
{
    if (!p->batched || batch < 1 || h < 1 || static_cast<int64_t>(batch) * h > 32 * kBatchedMaxTiles) return false;
    const int tiles = (batch * h + 31) / 32;
    return tiles * p->b_nw <= cus;
}

// basic_scanline_wavefront_max: the largest batch the schedule serves for a latent `h` rows high
inline int wavefront_max_batch(const ScanGeometry *p, int h, int cus)
{
    for (int b = 32 * kBatchedMaxTiles / h; b >= 1; --b)
        if (wavefront_fits(p, b, h, cus)) return b;
    return 0;
}

// The encode calls that take the wavefront schedule when nothing forces a choice: those with at most half the raster schedule's
// steps.  Measured (profiles/scanline_wavefront_probe.txt): a wavefront step costs 17.5-20.5 us at any
// shape that fits, a raster step 11.1-11.5 (pipelined, one image), 15.9 (two) or 16.3-17.2 (batched), so every call under this
// rule measured at least 1.38 times faster (run-to-run spread: 1 %); between half and 0.56 of the steps the wavefront still
// won by 11-19 %, above that the raster schedule is faster and stays.
inline bool wavefront_auto(const ScanGeometry *p, int batch, int h, int w)
{
    (void)batch;
    return 2 * wavefront_steps(p, h, w) <= static_cast<int64_t>(h) * w;
}

// ---- wavefront decode launch (row streams only): the wavefront's columns, plus one decoder wavefront per stream -- batch * h * lanes
// of them, four to a workgroup, resident beside the compute workgroups.
inline bool wavefront_decode_fits(const ScanGeometry *p, int batch, int h, int lanes, int cus)
{
    if (!wavefront_fits(p, batch, h, cus)) return false;
    const int tiles = (batch * h + 31) / 32;
    return static_cast<int64_t>(tiles) * p->b_nw + decoder_workgroups(batch * h * lanes) <= cus;
}

// The row-stream decode calls that take the wavefront launch when nothing forces a choice: none yet.  The rule is to be the encode
// rule (wavefront_auto: at most half the raster steps) cut down to the shapes where the launch MEASURED faster than the raster
// decode launch of the same shape and lane count by more than the run-to-run spread.  Its step is new -- the batched kernel's
// wavefront step (17.5-20.5 us in the encode launch) plus an in-loop decode of lane_w symbols per stream -- and no step cost has
// been measured (scripts/scanline_probe.py --rows measures it), so until one is, only
// BASIC_SCAN_KERNEL=wavefront sends a call here and auto keeps every row-stream call on the raster kernels.
inline bool wavefront_decode_auto(const ScanGeometry *p, int batch, int h, int w, int lanes)
{
    (void)p; (void)batch; (void)h; (void)w; (void)lanes;
    return false;
}

// ---- band encode schedule of the batched kernel (see the band section in front of it): an image owns band_slots() lanes of one
// column tile whatever its height, so a launch of T tiles codes T * (32 / slots) images in the wavefront's W + s (H - 1) steps, and
// a larger batch is coded by successive launches over whole images.
// kBandMaxTiles: a launch may hold cus / b_nw tiles (8 on a 256-unit chip with BaSIC's layers); every tile is one more set of b_nw
// resident workgroups that other streams' persistent launches queue behind (ScanChain).  Tiles share nothing but the memory side:
// measured (profiles/scanline_band_probe.txt), a step costs 18.4 us with one tile, 19.7 with two, 21.0 with four, 23.2-25.7 with
// eight, so halving the launches always won over the dearer step -- 64 / 96 images of 16x16: 8.99 / 12.03 ms at two tiles per
// launch, 4.78 / 6.37 at four, 3.52 / 3.90 at eight; 16x32x48: 13.1 / 7.0 / 4.3 ms.  8 = the whole chip.
constexpr int kBandMaxTiles = 8;
constexpr size_t kBandMaxScratch = static_cast<size_t>(1) << 30;   // bytes of scratch one band launch may ask for

inline int band_slots(const ScanGeometry *p, int w) { return w / wavefront_slope(p) + 1; }

// MFMA columns of a launch of the batched family that codes `images` images
inline int batched_columns(const ScanGeometry *p, ScanKernel mode, int images, int h, int w)
{
    if (mode == ScanKernel::kBatched) return images;
    if (mode == ScanKernel::kWavefront) return images * h;
    const int ipt = 32 / band_slots(p, w);
    return 32 * ((images + ipt - 1) / ipt);
}

// The images one band launch codes of an h x w latent: 0 = never (layers not of the batched kernel's shape, an image's slots do not
// fit one column tile, no tile's workgroups fit the chip, or one image alone is too large).  Limited by the tiles of a launch, by
// the scratch, and by the 32-bit element offsets the kernel computes: into y / sym / idx / ybuf of the launch's images
// (images * C * H * W), into a slab of the coded latent and into a step's slab of the prior (bytes).
inline int band_images_per_launch(const ScanGeometry *p, int h, int w, int cus)
{
    if (!p->batched || h < 1 || w < 1 || p->b_nw < 1) return 0;
    const int A = band_slots(p, w);
    if (A > 32) return 0;
    const int ipt = 32 / A, tiles_max = std::min(kBandMaxTiles, cus / p->b_nw);
    const int64_t steps = wavefront_steps(p, h, w);
    if (steps >= (1 << 30)) return 0;
    for (int n = tiles_max * ipt; n >= 1; --n) {
        const int tiles = (n + ipt - 1) / ipt;
        const int64_t yw = static_cast<int64_t>(n) * (h + p->ksize / 2);
        if (static_cast<int64_t>(n) * p->C * h * w >= (1ll << 31)) continue;
        if (yw * p->C * 8 >= (1ll << 31) || static_cast<int64_t>(tiles) * 32 * std::max(p->P, 1) * 4 >= (1ll << 31)) continue;
        if (batched_scratch(p, 32 * tiles, steps, static_cast<int>(yw), ScanKernel::kBand).total * sizeof(float) > kBandMaxScratch) continue;
        return n;
    }
    return 0;
}

// ---- band decode launch (row streams only): the band's compute workgroups, plus one decoder wavefront per (image, slot, lane
// stream) -- a slot's wavefront decodes the slot's rows one after the other, so an image brings min(band_slots, h) * lanes of them
// whatever its height --, four to a workgroup, resident beside the compute workgroups.  The images of one launch: the largest
// n <= band_images_per_launch whose tiles' workgroups and decoder workgroups together fit the chip; 0 = never.  (The decoder's
// search image must fit the LDS as for every decode launch: plan_scan checks it, the launch's LDS is the larger of the two.)
// Measured (scripts/scanline_probe.py --rows --decode-schedule band, profiles/band_decode_probe.txt; C = 192, 256 compute units,
// launch time / steps, run-to-run spread under 0.7 %): the step is the decoder wave's, not the band encode step's 18-26 us -- 64.4 us
// (one image of 32x48, one tile) to 67.4 (8 images, four tiles) and 68.1 - 70.8 (launches of six tiles) with one lane stream,
// 35.3 / 38.1 / 38.5 - 39.6 with three; the wavefront decode launch 64.8 - 65.3 / 35.6 - 36.2 where it fits.  The raster decode
// launches of the same row-stream calls: 51.2 / 25.2 us per step pipelined (one image; 56.8 / 30.6 two), 60.8 - 65.6 / 34.3 - 37.5
// batched.  So a call wins by its step count: 1 / 2 / 3 / 8 x 32x48 (172 steps against 1,536) x7.1 / x7.7 / x8.2 / x8.3 at one lane
// and x6.4 / x7.5 / x8.3 / x8.2 at three, 16 x 32x48 (two launches) x4.1, 64 x 16x16 (76 steps against 256, two / three launches)
// x1.56 / x1.06; no measured shape lost.  No auto rule is installed from these yet (a later change decides it and re-records the
// dispatch table): only the decode schedule or BASIC_SCAN_KERNEL=band sends a call here.
inline int band_decode_slots(const ScanGeometry *p, int h, int w) { return std::min(band_slots(p, w), h); }

inline int band_decode_images_per_launch(const ScanGeometry *p, int h, int w, int lanes, int cus)
{
    if (lanes < 1) return 0;
    const int most = band_images_per_launch(p, h, w, cus);
    if (most < 1) return 0;
    const int ipt = 32 / band_slots(p, w);
    const int64_t waves = static_cast<int64_t>(band_decode_slots(p, h, w)) * lanes;   // decoder wavefronts per image
    for (int n = most; n >= 1; --n)
        if (static_cast<int64_t>((n + ipt - 1) / ipt) * p->b_nw + (n * waves + kThreads / 64 - 1) / (kThreads / 64) <= cus) return n;
    return 0;
}

// The encode calls that take the band when nothing forces a choice and the wavefront does not fit.  Measured
// (profiles/scanline_band_probe.txt): a band step costs 17.9-18.4 us with one tile in the launch, 19.1-19.8
// with two, 20.1-21.0 with four, 23.2-25.7 with eight (more granules in flight through the same memory side); a raster step
// 11.1 us (pipelined, one image) or 16.1-17.7 (batched); run-to-run spread at most 0.7 %.
//   * One or two images (too tall for the wavefront): one tile, the wavefront's kernel step against the pipelined kernel's -- the
//     wavefront's measured rule, at most half the raster steps (1x135x120: 656 steps against 16,200, x15.2).
//   * Three images and more: the band is faster for certain while launches * steps * 25.7 <= H * W * 16.1 (its dearest step
//     against the cheapest batched raster step), i.e. launches * steps <= 0.625 H * W: alone on the chip every measured call under
//     that rule won by at least x1.29 (64x16x16: two launches, 152 steps against 256, 4.54 -> 3.52 ms; 3 / 8 / 16 x 32x48: x7.5 /
//     x7.2 / x5.9).  Alone is not how the coder runs, though: bench.py --workload basic (64x16x16, six stream workers) LOST with the
//     band, 183-190 -> 155-174 Mpix/s, three alternating runs each -- its first launch holds all 256 compute units for 1.8 ms
//     where the raster launch holds 64 for 4.5, and the other workers' launches queue behind it (ScanChain).  So the band must
//     also hold no more compute-unit time than the raster launch it replaces: tiles * steps summed over its launches, at 25.7 us,
//     against the raster launch's tiles * H * W at 16.1.  That leaves 64x16x16 (11 tile-launches of 76 steps against 2 x 256) and
//     16x32x48 (8 x 172 against 1,536) to raster and sends 3x32x48 and 8x32x48 to the band; whatever runs beside such a launch
//     then gets the chip sooner and no smaller.
// Batches that no raster kernel serves (more than 64 images) come here only when the coder's gate has already chosen the band over
// its per-step path (band_beats_per_step).
inline bool band_auto(const ScanGeometry *p, int batch, int h, int w, int per_launch)
{
    const int64_t launches = (batch + per_launch - 1) / per_launch, steps = wavefront_steps(p, h, w), hw = static_cast<int64_t>(h) * w;
    if (batch <= 2) return 2 * launches * steps <= hw;
    const int ipt = 32 / band_slots(p, w), last = batch - static_cast<int>(launches - 1) * per_launch;
    const int64_t tiles = (launches - 1) * ((per_launch + ipt - 1) / ipt) + (last + ipt - 1) / ipt;   // column tiles over all launches
    return 8 * launches * steps <= 5 * hw && 8 * tiles * steps <= 5 * hw * ((batch + 31) / 32);
}

// Auto, a batch no raster kernel serves: the band against the coder's per-step path.  Measured (scripts/scanline_band_probe.py,
// profiles/scanline_band_probe.txt): a band step costs at most 25.7 us (eight tiles in the launch), a step of the per-step
// path 110 us at 96 images (and more with the batch), so the band wins while launches * steps <= 4.3 H W; 3 leaves a
// margin (96x16x16: two launches, 152 steps against 256, 28.1 -> 3.9 ms).
inline bool band_beats_per_step(const ScanGeometry *p, int batch, int h, int w, int per_launch)
{
    if (per_launch < 1) return false;
    const int64_t launches = (batch + per_launch - 1) / per_launch;
    return launches * wavefront_steps(p, h, w) <= 3 * static_cast<int64_t>(h) * w;
}

// (kept as it is: the coder's residency gate counts the generic kernel's workgroups whichever kernel will run)
inline bool lane_grid_resident(const ScanGeometry *p, int ndec, int cus) { return p->nwg + ndec <= cus; }

// ---- The planner: the one place that decides how a scan-line call runs.  Pure: it asks nothing of the device or the environment.
struct ScanRequest {
    int batch = 1, h = 0, w = 0;     // h or w < 1: not known -- no kernel of the batched family is considered then
    int lanes = 1;                   // decode: lane streams per image (a decoder wavefront each); encode launches do not depend on it
    bool rows = false;               // decode: the row-stream format (batch * h * lanes streams): the wavefront launch may serve the call
    int table_len = 1;
    bool decode = false;
    bool fast_image = false;         // decode: the table set has a fast search image ...
    size_t decoder_lds = 0;          // ... of this many LDS bytes per decoder workgroup
    int cus = 0;                     // compute units of the device
    int schedule = BASIC_SCAN_SCHEDULE_AUTO;     // the requested encode schedule (decode calls ignore it)
    int decode_schedule = BASIC_SCAN_SCHEDULE_AUTO;   // the requested decode schedule: looked at only when the call brings row streams (rows)
    ScanKernel force = ScanKernel::kNone;        // BASIC_SCAN_KERNEL, parsed: wins over the schedule
    // the coder's gates (pgm_coder: persistent_scanline_max_batch): batches up to this one may take the lane kernels, and a call
    // that no persistent kernel should serve is left to the per-step path.  < 0: a library call, which is served or refused.
    int lane_max_batch = -1;
};

struct ScanLaunch {
    ScanKernel kernel = ScanKernel::kNone;   // kNone: leave the call to the per-step path
    int launches = 0, images = 0;            // `launches` launches over `images` whole images each (the last one: what is left)
    int grid = 0;                            // workgroups of a launch of `images` images: compute, then the decoder's
    size_t lds_bytes = 0;
    ScanLaneLds lane;                        // kGeneric, kPipelined: the LDS layout
    int cus = 0;
};

// compute workgroups of one launch over `images` images (resident: *_fits, band_images_per_launch and the lane check say so)
inline int compute_workgroups(const ScanGeometry *p, ScanKernel k, int images, int h, int w)
{
    if (k == ScanKernel::kGeneric || k == ScanKernel::kPipelined) return p->nwg;
    return ((batched_columns(p, k, images, h, w) + 31) / 32) * p->b_nw;
}

// Which kernel (the batched one from 3 images on where it fits, else the pipelined one where it fits, else the generic one;
// `force` names one, with identical results), in how many launches, with which grid and LDS.
// Encode calls have a second schedule, the wavefront one of the batched kernel: forced by BASIC_SCAN_KERNEL=wavefront or by the
// requested schedule (the environment wins), taken in auto where wavefront_auto says so; the raster schedule is the choice
// above, whatever wavefront_auto says.  Decode calls ignore both -- unless the call brings row streams (q.rows): then
// BASIC_SCAN_KERNEL=wavefront forces the wavefront decode launch, and auto takes it where wavefront_decode_fits and
// wavefront_decode_auto say so; where it does not fit, the raster kernels read the row streams (decoder workgroups of batch * lanes
// streams, as without rows), then the per-step path.  With rows off every request is planned as before the format existed.
// And a third, the band (BASIC_SCAN_KERNEL=band, BASIC_SCAN_SCHEDULE_BAND): any batch and height, in as many launches as the
// batch needs.  In auto it is looked at only where the wavefront does not fit, and taken where band_auto says so.
// Row-stream decode calls have a schedule of their own (ScanRequest::decode_schedule): auto is the above; raster keeps the call off the
// wavefront and the band whatever a later auto rule says; wavefront and band force that launch, as BASIC_SCAN_KERNEL=wavefront / band
// do (the environment wins).  The band decode launch (band_decode_images_per_launch) serves any batch and height, in as many
// launches as the batch needs, each with the decoder workgroups of its own images.  No auto rule sends a call to it.
// A forced kernel or schedule that the call does not fit is refused (BASIC_ERR_INVALID, "does not fit").
inline int plan_scan(const ScanGeometry *p, const ScanRequest &q, ScanLaunch *L)
{
    *L = ScanLaunch{};
    L->cus = q.cus;
    const bool decode = q.decode;
    const int batch = q.batch, h = q.h, w = q.w, cus = q.cus;
    const int ndec = decode ? decoder_workgroups(batch * q.lanes) : 0;
    int schedule = q.schedule;
    ScanKernel force = q.force;
    // encode only: a decode call ignores it (the wavefront and the band: unless it brings row streams)
    if (decode && force != ScanKernel::kNone && !scan_kernel_decodes(force, q.rows)) force = ScanKernel::kNone;
    // a row-stream decode call: its own schedule, where the environment names no kernel
    const int dsched = decode && q.rows ? q.decode_schedule : BASIC_SCAN_SCHEDULE_AUTO;
    if (force == ScanKernel::kNone && dsched == BASIC_SCAN_SCHEDULE_WAVEFRONT) force = ScanKernel::kWavefront;
    if (force == ScanKernel::kNone && dsched == BASIC_SCAN_SCHEDULE_BAND) force = ScanKernel::kBand;
    const bool wf_fits = decode ? q.rows && h >= 1 && w >= 1 && wavefront_decode_fits(p, batch, h, q.lanes, cus) && q.decoder_lds <= kMaxLds
                                : wavefront_fits(p, batch, h, cus);
    // a row-stream decode call that goes to the wavefront launch: forced, or in auto where it fits and its rule says so
    const bool wf_decode = decode && wf_fits && (force == ScanKernel::kWavefront || (force == ScanKernel::kNone && dsched == BASIC_SCAN_SCHEDULE_AUTO && wavefront_decode_auto(p, batch, h, w, q.lanes)));
    // a row-stream decode call whose band launch was asked for: the images of one launch (0: it does not fit)
    const bool band_decode = decode && force == ScanKernel::kBand;
    const int band_dec_n = band_decode && h >= 1 && w >= 1 && q.decoder_lds <= kMaxLds ? band_decode_images_per_launch(p, h, w, q.lanes, cus) : 0;
    int band_n = -1;   // band_images_per_launch, when somebody asks
    auto band_images = [&] { return band_n >= 0 ? band_n : (band_n = band_images_per_launch(p, h, w, cus)); };
    if (q.lane_max_batch >= 0) {
        if (decode && !q.fast_image) return BASIC_OK;
        // a forced band serves any batch: the call is cut into launches over whole images
        const bool band_asked = !decode && schedule == BASIC_SCAN_SCHEDULE_BAND && band_images() >= 1;
        if (!band_asked && batch > q.lane_max_batch && batch > batched_max_batch(p, w, decode, cus, q.lanes)) {
            // no raster kernel serves this batch; an encode call may still run as a wavefront (a narrow latent, for one), or, in
            // auto, as a band where that beats the per-step path.  (kept as it is: a forced wavefront that does not fit is not
            // refused here but left to the per-step path)
            if (decode) {
                if (!wf_decode && band_dec_n < 1) return BASIC_OK;   // (row streams: the wavefront or band decode launch serves the call, chosen below)
            } else if (schedule == BASIC_SCAN_SCHEDULE_RASTER) return BASIC_OK;
            else if (wf_fits) schedule = BASIC_SCAN_SCHEDULE_WAVEFRONT;
            else if (schedule == BASIC_SCAN_SCHEDULE_AUTO && band_beats_per_step(p, batch, h, w, band_images())) schedule = BASIC_SCAN_SCHEDULE_BAND;
            else return BASIC_OK;
        }
        if (!wf_decode && band_dec_n < 1 && (!lane_grid_resident(p, ndec, cus) || (decode && q.decoder_lds > kMaxLds))) return BASIC_OK;
    }
    if (force == ScanKernel::kNone && !decode && schedule == BASIC_SCAN_SCHEDULE_WAVEFRONT) force = ScanKernel::kWavefront;
    if (force == ScanKernel::kNone && !decode && schedule == BASIC_SCAN_SCHEDULE_BAND) force = ScanKernel::kBand;
    const bool automatic = force == ScanKernel::kNone && schedule == BASIC_SCAN_SCHEDULE_AUTO;
    const bool fits = batched_fits(p, batch, w, ndec, cus);
    if (force == ScanKernel::kBatched) BASIC_REQUIRE(fits, "scanline: BASIC_SCAN_KERNEL=batched, but this call does not fit the batched kernel");
    if (force == ScanKernel::kWavefront) BASIC_REQUIRE(wf_fits, decode ? "scanline: the wavefront decode launch was asked for, but this row-stream decode call does not fit the wavefront launch"
                                                                       : "scanline: the wavefront encode schedule was asked for, but this call does not fit it");
    const int per_launch = decode ? band_dec_n : (force == ScanKernel::kBand || (automatic && !wf_fits)) ? band_images() : 0;
    if (force == ScanKernel::kBand) BASIC_REQUIRE(per_launch >= 1, decode ? "scanline: the band decode launch was asked for, but this row-stream decode call does not fit it"
                                                                          : "scanline: the band encode schedule was asked for, but this call does not fit it");
    L->images = batch;
    if (force == ScanKernel::kBand || (per_launch >= 1 && band_auto(p, batch, h, w, per_launch))) {
        L->kernel = ScanKernel::kBand;
        L->images = std::min(per_launch, batch);
    } else if (force == ScanKernel::kWavefront || wf_decode || (!decode && automatic && wf_fits && wavefront_auto(p, batch, h, w))) {
        L->kernel = ScanKernel::kWavefront;
    } else if (force == ScanKernel::kBatched || (force == ScanKernel::kNone && fits && batch >= 3)) {
        L->kernel = ScanKernel::kBatched;
    } else {
        const int rc = lane_lds(p, batch, w, q.table_len, force, &L->lane);
        if (rc) return rc;
        L->kernel = L->lane.pipelined ? ScanKernel::kPipelined : ScanKernel::kGeneric;
        L->lds_bytes = L->lane.lds_bytes;
        BASIC_REQUIRE(p->nwg + ndec <= cus, "scanline: more workgroups than compute units (the grid must be resident)");
    }
    if (L->kernel != ScanKernel::kGeneric && L->kernel != ScanKernel::kPipelined)
        L->lds_bytes = (align4(q.table_len) + 4 + 96 + static_cast<size_t>(p->b_tiles) * kBTile) * sizeof(float);   // table, flags, biases, partial tiles
    L->launches = (batch + L->images - 1) / L->images;
    // (the wavefront decode launch: a decoder wavefront per row stream; the band decode launch: one per slot and lane of its images)
    L->grid = compute_workgroups(p, L->kernel, L->images, h, w) +
              (decode && L->kernel == ScanKernel::kWavefront ? decoder_workgroups(batch * h * q.lanes)
               : decode && L->kernel == ScanKernel::kBand    ? decoder_workgroups(L->images * band_decode_slots(p, h, w) * q.lanes)
                                                             : ndec);
    if (decode) L->lds_bytes = std::max(L->lds_bytes, q.decoder_lds);
    if (L->lds_bytes < kMinLds) L->lds_bytes = kMinLds;
    BASIC_REQUIRE(L->lds_bytes <= kMaxLds, L->kernel == ScanKernel::kBand ? "scanline: a workgroup's LDS does not fit"
                                                                          : "scanline: a workgroup's LDS (decoder: the search image) does not fit");
    return BASIC_OK;
}

// lane streams: `lanes` runs of C / lanes channels, each a multiple of 16 (see decoder_workgroup); 1 = one stream per image
inline bool valid_lanes(const ScanGeometry *p, int lanes) { return lanes == 1 || (lanes > 1 && p->C % lanes == 0 && (p->C / lanes) % 16 == 0); }

}  // namespace basic
