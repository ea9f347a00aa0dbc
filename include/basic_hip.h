/*
 * basic_hip.h -- C ABI of libbasic_hip.so, the MI355X (gfx950) native replacement for the
 * native layer of worldlife123/cbench_BaSIC on the encode/decode hot path.
 *
 * Every entry point is `extern "C"`, takes plain pointers / sizes, returns an int status and
 * never throws.  Pointers named d_* are DEVICE pointers (HBM); everything else is host
 * memory.  `hip_stream` is a hipStream_t passed as void* (NULL = default stream).
 * Citations (file:line) are relative to the reference checkout /root/reference.
 */
#ifndef BASIC_HIP_H
#define BASIC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (the Python shim maps them to the reference's exceptions) ---------- */
#define BASIC_OK 0
#define BASIC_ERR_INVALID (-1)   /* py::value_error in the reference (bad shape/argument)      */
#define BASIC_ERR_NOT_INIT (-2)  /* "ANS not initialized!"  csrc/ans/rans64.cpp:209,395,506   */
#define BASIC_ERR_HIP (-3)       /* HIP runtime failure; text in basic_last_error()            */
#define BASIC_ERR_OVERFLOW (-4)  /* caller buffer too small (reference: UB, rans64.cpp:240)    */
#define BASIC_ERR_NO_DEVICE (-5) /* no gfx950 device visible: the library never falls back     */

const char *basic_last_error(void);
/* Number of visible HIP devices; BASIC_ERR_NO_DEVICE if none. */
int basic_device_count(int *count);
int basic_set_device(int ordinal);
int basic_stream_synchronize(void *hip_stream);

/* ======================================================================================
 * 1. rANS tables  -- replaces Rans64Base::init_params / init_cdf_params / get_cdfs
 *    (csrc/ans/rans64.cpp:69-182, rans64.hpp:38-49) and pmf_to_quantized_cdf
 *    (csrc/ans/rans64.cpp:69-126 == csrc/rans/rans_interface.cpp:450-519).
 *    Tables are built on the host in IEEE float32 with the reference's operation order and
 *    uploaded once; the object owns both copies.
 * ==================================================================================== */
typedef struct basic_rans_tables basic_rans_tables;

int basic_pmf_to_quantized_cdf(const float *pmf, int n, int precision, int32_t *cdf_out /* n+1 */);

/* freqs: int32 [rows][freq_stride]; nsym/offsets: int32 [rows]. */
int basic_rans_tables_from_freqs(const int32_t *freqs, int rows, int freq_stride, const int32_t *nsym,
                                 const int32_t *offsets, int freq_precision, int bypass_coding,
                                 int bypass_precision, basic_rans_tables **out);
/* cdfs: int32 [rows][cdf_stride]; cdf_sizes/offsets: int32 [rows]. */
int basic_rans_tables_from_cdfs(const int32_t *cdfs, int rows, int cdf_stride, const int32_t *cdf_sizes,
                                const int32_t *offsets, int freq_precision, int bypass_coding,
                                int bypass_precision, basic_rans_tables **out);
/* AR index-remap tables, ANSBase::init_ar_params (csrc/ans/ans_interface.cpp:75-137):
 * ar_tab int32 [k][rows][s1] (order 1) or [k][rows][s1][s1] (order 2). */
int basic_rans_tables_set_ar(basic_rans_tables *t, const int32_t *ar_tab, int k, int rows, int order, int s1);
/* Custom AR ops, ANSBase::init_custom_ar_ops (csrc/ans/ans_interface.hpp:40-48; the op: ar_limited_scaled_add_linear_op,
 * csrc/ans/ar_funcs.hpp:58-87): ops float32 [k][7] = (w0, w1, w2, bias, scale, min, max).  The table row of an element becomes
 * op(index, previous symbols) -- RAW symbol values at the back distances of the call's ar_offsets rows (1..3 of them). */
int basic_rans_tables_set_ar_ops(basic_rans_tables *t, const float *ops, int k);
int basic_rans_tables_info(const basic_rans_tables *t, int *rows, int *max_cdf_len);
/* get_cdfs(): out int32 [rows][out_stride], padding written as 0. */
int basic_rans_tables_get_cdfs(const basic_rans_tables *t, int32_t *out, int out_stride);
/* Bit cost of every table symbol in units of 2^-16 bit (rate control, section 4): pure host code, no device.
 *     out[r][v] = llrint((precision - log2(cdf[r][v + 1] - cdf[r][v])) * 65536)   in double, v <= cdf_sizes[r] - 2; 0 beyond
 * cdfs int32 [rows][stride], out uint32 [rows][stride].  A frequency that is not positive: BASIC_ERR_INVALID. */
int basic_rans_cost_table_host(const int32_t *cdfs, int rows, int stride, const int32_t *cdf_sizes, int precision, uint32_t *out);
/* The cost table of a table set, uint32 [rows][max_cdf_len] (basic_rans_tables_info), as the rate kernels read it.  A set builds
 * and uploads it on the first rate call (or here): sets that are never rated hold nothing for it. */
int basic_rans_tables_costs(const basic_rans_tables *t, uint32_t *host_out);
void basic_rans_tables_destroy(basic_rans_tables *t);

/* ======================================================================================
 * 2. Host-buffer coder -- the drop-in for the pybind11 methods
 *      Rans64Encoder::encode_with_indexes   csrc/ans/rans64.cpp:203-361
 *      Rans64Decoder::decode_with_indexes   csrc/ans/rans64.cpp:389-499
 *      Rans64Decoder::set_stream/decode_stream  rans64.hpp:104-111, rans64.cpp:501-598
 *      BufferedRansEncoder/RansDecoder      csrc/rans/rans_interface.cpp:109-424
 *    Arrays are staged to HBM, coded by the HIP kernel, and the result copied back.
 *    ar_indexes may be NULL (treated as 0); ar_off0/ar_off1 are the per-element back
 *    distances (rows of the reference's ar_offsets array); pass NULL when no AR table is set.
 * ==================================================================================== */
int basic_rans_encode_host(const basic_rans_tables *t, const int32_t *symbols, const int32_t *indexes,
                           int64_t n, const int32_t *ar_indexes, const int32_t *ar_off0,
                           const int32_t *ar_off1, uint8_t *out, int64_t out_capacity, int64_t *out_len);
/* The same with a third ar_offsets row (custom AR ops take up to three predecessors). */
int basic_rans_encode_host_ex(const basic_rans_tables *t, const int32_t *symbols, const int32_t *indexes, int64_t n,
                              const int32_t *ar_indexes, const int32_t *ar_off0, const int32_t *ar_off1,
                              const int32_t *ar_off2, uint8_t *out, int64_t out_capacity, int64_t *out_len);
/* The same with the table rows taken as given even when the set carries an AR remap: Rans64Encoder::flush() of symbols that AR
 * calls cached -- their rows were remapped when they were cached (rans64.cpp:258-263,343,363-386). */
int basic_rans_encode_host_rows(const basic_rans_tables *t, const int32_t *symbols, const int32_t *indexes, int64_t n,
                                uint8_t *out, int64_t out_capacity, int64_t *out_len);
int basic_rans_decode_host_ex(const basic_rans_tables *t, const uint8_t *stream, int64_t stream_len, const int32_t *indexes,
                              int64_t n, const int32_t *ar_indexes, const int32_t *ar_off0, const int32_t *ar_off1,
                              const int32_t *ar_off2, int32_t *out_symbols);
/* Upper bound of the encoded size in bytes for n symbols (always sufficient). */
int64_t basic_rans_encode_bound(int64_t n);
int basic_rans_decode_host(const basic_rans_tables *t, const uint8_t *stream, int64_t stream_len,
                           const int32_t *indexes, int64_t n, const int32_t *ar_indexes,
                           const int32_t *ar_off0, const int32_t *ar_off1, int32_t *out_symbols);

/* Host framing of a batch of per-image streams, the wire format of CompressAI-style coders
 * (reference: write_body / read_body, cbench/modules/prior_model/prior_coder/compressai_coder.py:63-84):
 * ">III" (h, w, n) then per stream ">I" byte length + payload.  `words` holds the n streams back to
 * back, stream i = words[word_off[i] .. word_off[i+1]).  frame: returns BASIC_ERR_OVERFLOW if
 * out_capacity is too small (needed size in *out_len).  unframe: word_off needs n+1 entries and
 * words_out (len - 12 - 4n) / 4 words; pass words_out = NULL to query h, w, n only. */
int basic_frame_streams(const uint32_t *words, const int64_t *word_off, int n, uint32_t h, uint32_t w,
                        uint8_t *out, int64_t out_capacity, int64_t *out_len);
int basic_unframe_streams(const uint8_t *data, int64_t len, uint32_t *h, uint32_t *w, int *n,
                          int64_t *word_off, int n_capacity, uint32_t *words_out);

typedef struct basic_rans_stream basic_rans_stream;
int basic_rans_stream_open(const basic_rans_tables *t, const uint8_t *stream, int64_t stream_len,
                           basic_rans_stream **out);
int basic_rans_stream_decode(basic_rans_stream *s, const int32_t *indexes, int64_t n, int32_t *out_symbols);
void basic_rans_stream_close(basic_rans_stream *s);

/* ======================================================================================
 * 3. Batched device-pointer coder (the hot path: one independent stream per image).
 *    d_seg[nstreams+1] (int64) gives each stream's symbol range inside d_symbols/d_indexes.
 *    Encoder: stream i is written right-aligned into its slot
 *       d_out_words[i*slot_words .. (i+1)*slot_words), its length in d_out_nwords[i]
 *       (-1 = slot overflow).  Bytes = little-endian u32 words, exactly the reference's
 *       py::bytes (rans64.cpp:352-354).
 *    Decoder: stream i is the words d_words[d_word_off[i] .. d_word_off[i+1]) (d_word_off has
 *       nstreams+1 entries; reads past a stream's end return 0 instead of faulting);
 *       d_state/d_pos (per stream) carry the coder between calls (decode_stream semantics);
 *       set d_pos[i] = -1 to initialise from the stream head.
 * ==================================================================================== */
int basic_rans_encode_batch_dev(const basic_rans_tables *t, const int32_t *d_symbols,
                                const int32_t *d_indexes, const int64_t *d_seg, int nstreams,
                                uint32_t *d_out_words, int64_t slot_words, int32_t *d_out_nwords,
                                void *hip_stream);
/* Packs the right-aligned encoder slots into one contiguous buffer: stream i (d_nwords[i] words)
 * goes to d_out + d_out_off[i]; streams with d_nwords[i] <= 0 are skipped. */
int basic_rans_compact_streams_dev(const uint32_t *d_slots, int64_t slot_words, const int32_t *d_nwords,
                                   const int64_t *d_out_off, int nstreams, uint32_t *d_out, void *hip_stream);
int basic_rans_decode_batch_dev(const basic_rans_tables *t, const uint32_t *d_words,
                                const int64_t *d_word_off, const int32_t *d_indexes, const int64_t *d_seg,
                                int nstreams, int32_t *d_out_symbols, uint64_t *d_state, int64_t *d_pos,
                                void *hip_stream);

/* Same decoder with arithmetic segments instead of a d_seg array: stream b decodes the `count` symbols whose
 * indexes sit at d_indexes[first + b*stride ...] and writes them at the same positions of d_out_symbols.  This is
 * the per-topo-group step of the AR coder (decode_stream, pgm_coder.py:971) on dense [B][n] arrays. */
int basic_rans_decode_batch_strided_dev(const basic_rans_tables *t, const uint32_t *d_words,
                                        const int64_t *d_word_off, const int32_t *d_indexes, int64_t first,
                                        int64_t stride, int64_t count, int nstreams, int32_t *d_out_symbols,
                                        uint64_t *d_state, int64_t *d_pos, void *hip_stream);
/* The same step for the LANE STREAMS of the scan-line coder (stream_lanes = `lanes`): nimages * lanes streams,
 * stream s = b * lanes + k continues with the `count` symbols whose indexes sit at d_indexes[first + b*stride + k*count ...]
 * (d_state / d_pos / d_word_off are indexed by s).  lanes == 1 is basic_rans_decode_batch_strided_dev; same kernel. */
int basic_rans_decode_batch_lanes_dev(const basic_rans_tables *t, const uint32_t *d_words, const int64_t *d_word_off,
                                      const int32_t *d_indexes, int64_t first, int64_t stride, int lanes, int64_t count,
                                      int nimages, int32_t *d_out_symbols, uint64_t *d_state, int64_t *d_pos, void *hip_stream);
/* basic_rans_decode_batch_lanes_dev with a stream base and stride, for the ROW STREAMS of the scan-line coder (stream_rows,
 * INTEGRATION.md): the launch's stream (b, k), b < nimages, k < lanes, is stream stream_first + b*stream_stride + k of d_word_off /
 * d_state / d_pos and continues with the `count` symbols at first + b*stride + k*count.  The coder calls it per position p with
 * stream_first = (p / W) * lanes, stream_stride = H * lanes.  stream_stride >= lanes; (0, lanes) is the lanes entry; same kernel. */
int basic_rans_decode_batch_streams_dev(const basic_rans_tables *t, const uint32_t *d_words, const int64_t *d_word_off,
                                        const int32_t *d_indexes, int64_t first, int64_t stride, int lanes, int64_t count,
                                        int nimages, int stream_first, int stream_stride, int32_t *d_out_symbols,
                                        uint64_t *d_state, int64_t *d_pos, void *hip_stream);

/* Which kernel the calling thread's last rANS launch was (host or device entry point, scan-line step decodes included), so
 * that a test can tell which of the table-dependent paths it ran.  ENC_FAST / DEC_FAST are the lane-parallel kernels, with
 * *waves = wavefronts (streams) per workgroup; the others run one wavefront per workgroup (*waves = 1).  LDS / GLOBAL: the
 * packed 16-bit rows are copied to the LDS, or searched in global memory (packed copy over 144 KiB). */
#define BASIC_RANS_KERNEL_NONE (-1) /* no launch by this thread yet */
#define BASIC_RANS_KERNEL_ENC_FAST 0
#define BASIC_RANS_KERNEL_ENC_GENERAL 1
#define BASIC_RANS_KERNEL_ENC_GENERAL_AR 2
#define BASIC_RANS_KERNEL_DEC_FAST 3
#define BASIC_RANS_KERNEL_DEC_GENERAL_LDS 4
#define BASIC_RANS_KERNEL_DEC_GENERAL_GLOBAL 5
#define BASIC_RANS_KERNEL_DEC_AR_LDS 6
#define BASIC_RANS_KERNEL_DEC_AR_GLOBAL 7
int basic_rans_last_launch(int *kernel, int *waves);
/* Wavefronts per workgroup of the fast kernels for the calling thread's launches: 1, 2, 4, 8 or 16; 0 hands the choice back to
 * the environment variable BASIC_RANS_WPB (read once per process; default 1), over which any other value takes precedence.
 * *previous (optional) = the value replaced.  A codec session sets it around its own launches (basic_hp_session_set_rans_waves). */
int basic_rans_set_waves(int waves_per_block, int *previous);

/* ======================================================================================
 * 4. Entropy-parameter kernels (coalesced elementwise, fused quantise + table index).
 * ==================================================================================== */
/* CompressAI GaussianConditional path (compressai_coder.py:377-393; upstream build_indexes
 * quoted at pgm_coder.py:814-818): idx = (T-1) - #{j<T-1 : max(scale,bound) <= table[j]},
 * sym = round_half_even(y).  d_table: float32 [T] on device.  d_yhat (optional) = float(sym). */
int basic_gc_quantize_index_dev(const float *d_y, const float *d_scales, int64_t n, const float *d_table,
                                int table_len, float scale_bound, int32_t *d_symbols, int32_t *d_indexes,
                                float *d_yhat, void *hip_stream);
/* Quantiser step (no reference counterpart; an opt-in format, INTEGRATION.md "Quantiser step").  Element i belongs to image
 * b = i / per_image and takes step = d_steps[n_steps == 1 ? 0 : b], float32 on the device.  Every line is one fp32 operation:
 *     s   = max(scale, bound)                 LowerBound first, as basic_gc_quantize_index_dev
 *     s'  = s / step                          IEEE division, correctly rounded (no reciprocal)
 *     idx = the index rule above on s'        (same search, same NaN / unsorted-table fallback)
 *     q   = round_half_even(y / step)         the same division
 *     sym = (int32) q,   yhat = q * step      one multiply; the decoder's (float) sym * step is the same bits for sym != 0
 *                                             (sym == 0: +0.0, where rint may have left the encoder -0.0, as without a step)
 * With every step 1 the outputs are those of basic_gc_quantize_index_dev / basic_i32_to_f32_dev bit for bit.  n must be a
 * whole number of images and n_steps 1 or n / per_image, else BASIC_ERR_INVALID.  The step VALUES live on the device and are
 * not inspected here: the caller validates them on the host (finite, in [BASIC_QSTEP_MIN, BASIC_QSTEP_MAX]) before it uploads
 * them, as basic_hp_session_set_qsteps does.  A decoder obtains its indexes from the same entry point with d_y = d_scales and
 * d_yhat = NULL (the symbols are scratch), the way the step-less decoder uses basic_gc_quantize_index_dev. */
#define BASIC_QSTEP_MIN 0.0625f /* 2^-4 */
#define BASIC_QSTEP_MAX 64.0f   /* 2^6  */
int basic_gc_quantize_index_q_dev(const float *d_y, const float *d_scales, int64_t n, int64_t per_image, const float *d_steps,
                                  int n_steps, const float *d_table, int table_len, float scale_bound, int32_t *d_symbols,
                                  int32_t *d_indexes, float *d_yhat, void *hip_stream);
/* d_yhat[i] = (float) d_sym[i] * step of image i / per_image: the encoder's yhat (bit for bit where d_sym[i] != 0). */
int basic_gc_dequantize_q_dev(const int32_t *d_sym, int64_t n, int64_t per_image, const float *d_steps, int n_steps,
                              float *d_yhat, void *hip_stream);
/* Rate control (no reference counterpart; INTEGRATION.md "Rate control"): what the rANS coder of table set t would spend on every
 * stream at each of n_cand candidate steps, from ONE read of y and the scales.  Segment s = image b, lane l -> b * segs_per_image + l
 * holds the per_seg contiguous elements from s * per_seg on, the streams of the batched encoder.  d_cand: float32 on the device,
 * [n_cand] shared by all images (cand_per_image == 0) or [n_seg / segs_per_image][n_cand] (cand_per_image == 1); the values are not
 * inspected here (the caller validates them on the host, as for d_steps above).  d_bits uint64 [n_seg][n_cand], cleared by the call:
 *     d_bits[s][k] = sum over the segment of cost(sym, idx),  (sym, idx) = what basic_gc_quantize_index_q_dev writes at step cand[k]
 *     value = sym - offset[idx], max = cdf_size[idx] - 2
 *     value < 0: raw = -2 value - 1;  value >= max: raw = 2 (value - max);  either way the symbol is escaped
 *     cost = table[idx][escaped ? max : value] + (escaped ? bypass_precision (nb + 1 + nb / maxbv) 65536 : 0)
 *     nb = digits of bypass_precision bits in raw, maxbv = 2^bypass_precision - 1;  table = basic_rans_cost_table_host's
 * in units of 2^-16 bit.  Integer sums: the result depends on neither the launch shape nor the order of arrival.
 * BASIC_ERR_INVALID: n_cand outside [1, 32], n_seg no multiple of segs_per_image, tables without bypass coding, with a precision
 * other than 16 or more than 1024 rows, per_seg * 2^22 past 63 bits. */
int basic_gc_rate_curve_dev(const float *d_y, const float *d_scales, int n_seg, int64_t per_seg, int segs_per_image, const float *d_cand,
                            int n_cand, int cand_per_image, const float *d_table, int table_len, float scale_bound,
                            const basic_rans_tables *t, uint64_t *d_bits, void *hip_stream);
/* Mean-scale (the y coder of the mean-scale hyperprior, upstream's MeanScaleHyperprior; INTEGRATION.md "Mean-scale hyperprior").
 * The parameters of element i, image b = i / per_image, r = i % per_image, lie at d_scales[b * param_stride + r] and
 * d_means[b * param_stride + r]: the halves of a chunked prior [B][2 M][h][w] are read in place with d_means = d_scales + per_image
 * and param_stride = 2 * per_image; two separate contiguous arrays have param_stride = per_image.  Every line one fp32 operation:
 *     s    = max(scale, bound)                    s' = s / step            (only with a step)
 *     idx  = the index rule above on s (or s')
 *     r    = y - mu
 *     q    = round_half_even(r)                   or round_half_even(r / step)
 *     sym  = (int32) q
 *     yhat = q + mu                               or (q * step) + mu: two roundings, never an FMA
 *     decoder (basic_gc_dequantize_ms_dev): yhat = (float) sym + mu   or ((float) sym * step) + mu
 * The decoder's yhat has the encoder's bits wherever sym != 0 or mu != 0 (at sym == 0 and mu == +-0 both are a zero).  With every
 * step 1 the outputs are the step-less ones bit for bit; with mu = +0.0 everywhere sym, idx and the value of yhat are those of
 * basic_gc_quantize_index_q_dev / basic_gc_quantize_index_dev.  n_steps == 0 or d_steps == NULL: the step-less lines (a kernel
 * without a division); else d_steps as above.  d_y == NULL with d_symbols == NULL and d_yhat == NULL: indexes only (the decoder;
 * d_means is not read).  BASIC_ERR_INVALID, before any launch: n no whole number of images, n_steps not in {0, 1, n / per_image},
 * param_stride < per_image, d_y without d_symbols or d_means, d_symbols or d_yhat without d_y. */
int basic_gc_quantize_index_ms_dev(const float *d_y, const float *d_scales, const float *d_means, int64_t n, int64_t per_image,
                                   int64_t param_stride, const float *d_steps, int n_steps, const float *d_table, int table_len,
                                   float scale_bound, int32_t *d_symbols, int32_t *d_indexes, float *d_yhat, void *hip_stream);
int basic_gc_dequantize_ms_dev(const int32_t *d_sym, const float *d_means, int64_t n, int64_t per_image, int64_t param_stride,
                               const float *d_steps, int n_steps, float *d_yhat, void *hip_stream);
/* basic_gc_rate_curve_dev for the mean-scale coder: (sym, idx) = what basic_gc_quantize_index_ms_dev writes at step cand[k].  The
 * parameters of segment s, image b = s / segs_per_image, start at b * param_stride + (s % segs_per_image) * per_seg of d_scales
 * and d_means; param_stride >= per_seg * segs_per_image, else BASIC_ERR_INVALID.  Everything else as above. */
int basic_gc_rate_curve_ms_dev(const float *d_y, const float *d_scales, const float *d_means, int64_t param_stride, int n_seg,
                               int64_t per_seg, int segs_per_image, const float *d_cand, int n_cand, int cand_per_image,
                               const float *d_table, int table_len, float scale_bound, const basic_rans_tables *t, uint64_t *d_bits,
                               void *hip_stream);
/* The step of every image from its curve.  A stream of n symbols whose costs sum to bits (2^-16 bit) takes at most
 * 2 + ((bits + 4 n) >> 21) 32-bit words (INTEGRATION.md "Rate control": the byte bound), so
 *     pred_bytes(b, k) = 4 extra_words[b] + sum over the lanes of 4 (2 + ((bits[s][k] + 4 per_seg) >> 21))
 * and d_choice[b] = the FIRST k in candidate order with pred_bytes(b, k) <= d_budget[b] (the curve need not be monotone); when none
 * fits, (n_cand - 1) | BASIC_RATE_NO_FIT.  d_steps_out[b] = the chosen candidate, d_pred_bytes[b] its prediction.  d_extra_words:
 * int32 [n_images] (e.g. the z streams' word counts) or NULL; d_budget int64 [n_images]. */
#define BASIC_RATE_NO_FIT 0x40000000
int basic_rate_select_dev(const uint64_t *d_bits, int n_images, int segs_per_image, int64_t per_seg, const float *d_cand, int n_cand,
                          int cand_per_image, const int32_t *d_extra_words, const int64_t *d_budget, float *d_steps_out,
                          int32_t *d_choice, int64_t *d_pred_bytes, void *hip_stream);
/* basic_rate_select_dev for GROUPS of tiles: a tiled picture (group g) has one budget over all its tiles, which lie in several
 * curve calls and need not share per_seg (INTEGRATION.md "Tiled pictures: step and byte budget").  Tile t owns the `lanes` rows
 * tile_first_seg[t] .. + lanes - 1 of d_bits uint64 [n_seg][n_cand], streams of tile_per_seg[t] symbols each; group g lists the tiles
 * group_tiles[group_first[g] .. group_first[g + 1]) (CSR; a tile belongs to at most one group, any order).
 *     pred(g, k) = sum over t in g of (4 extra_words[t] + sum over the lanes of 4 (2 + ((bits[s][k] + 4 per_seg[t]) >> 21)))
 * d_choice[g] = the FIRST k in candidate order with pred(g, k) <= d_budget[g]; none: (n_cand - 1) | BASIC_RATE_NO_FIT.
 * d_steps_out[g] = the chosen candidate (d_cand float32 [n_cand], or [n_groups][n_cand] with cand_per_group == 1), d_pred_bytes[g] =
 * its prediction; d_tile_steps[t] / d_tile_pred[t] = the group's step and the tile's own term of the sum at the chosen k, for every
 * listed tile (the others are not written).  d_tile_steps is what basic_gc_quantize_index_q_dev reads as one step per image.
 * The four plan arrays are HOST arrays: they are checked here and uploaded (stream-ordered) into d_plan, device memory of at least
 * BASIC_RATE_GROUPS_PLAN_BYTES(n_tiles, n_groups) bytes, 8-byte aligned, which the kernel reads -- it never sees an unchecked index.
 * d_tile_extra_words: int32 [n_tiles] on the device, or NULL.  One workgroup of block_threads (0: 256; else a multiple of 64 up to
 * 1024) per group; integer sums, so the result depends on neither.  BASIC_ERR_INVALID, before anything is enqueued: a null pointer,
 * n_cand outside [1, 32], lanes / n_seg / n_tiles / n_groups < 1, a tile whose rows leave d_bits or whose per_seg * 2^22 passes 63
 * bits, an empty group, a tile index out of range or listed twice, a bad block_threads. */
#define BASIC_RATE_GROUPS_PLAN_BYTES(n_tiles, n_groups) (16 * (size_t)(n_tiles) + 4 * ((size_t)(n_groups) + 1))
int basic_rate_select_groups_dev(const uint64_t *d_bits, int n_seg, int lanes, int n_tiles, const int32_t *host_tile_first_seg,
                                 const int64_t *host_tile_per_seg, const int32_t *d_tile_extra_words, int n_groups,
                                 const int32_t *host_group_first, const int32_t *host_group_tiles, void *d_plan, const float *d_cand,
                                 int n_cand, int cand_per_group, const int64_t *d_budget, float *d_steps_out, int32_t *d_choice,
                                 int64_t *d_pred_bytes, float *d_tile_steps, int64_t *d_tile_pred, int block_threads, void *hip_stream);
/* The next grid, d_cand_out float32 [n_images][n_cand], between the chosen candidate k and the one below it.  k == 0 or no fit:
 * every entry is the chosen step (the image is settled).  Otherwise lo = cand[k - 1], hi = cand[k] and
 *     cand_out[j] = fminf(lo + (hi - lo) * t[j], hi)  for j < n_cand - 1,   cand_out[n_cand - 1] = hi
 * subtract, multiply and add each one fp32 operation.  d_t float32 [n_cand] (the caller's (j + 1) / n_cand). */
int basic_rate_refine_dev(const float *d_cand_in, int cand_per_image, int n_cand, const int32_t *d_choice, int n_images,
                          const float *d_t, float *d_cand_out, void *hip_stream);
/* Lane streams of the scan-line coder: repacks d_sym / d_idx, int32 [B][positions][channels] in coding order, to
 * [B][lanes][positions][channels / lanes] (lane k = channels [k L, (k + 1) L), L = channels / lanes), so that
 * basic_rans_encode_batch_dev codes B * lanes contiguous streams of positions * L symbols.  Out of place; lanes == 1 copies. */
int basic_lanes_pack_dev(const int32_t *d_sym, const int32_t *d_idx, int batch, int positions, int channels, int lanes,
                         int32_t *d_sym_out, int32_t *d_idx_out, void *hip_stream);
/* Lane streams of the group coders (GaussianConditional: groups == 1; topo-group coders: the plan's groups): repacks d_sym /
 * d_idx, int32 [B][n] in group-major coding order, to [B][lanes][n / lanes], where stream (b, k) is the concatenation over the
 * groups g of the k-th of `lanes` equal contiguous parts of group g.  d_bases: int64 [groups + 1] on the device, the first
 * element of every group and n at the end; every group must be a multiple of `lanes` long (groups may be empty, and of unequal
 * lengths).  Out of place; lanes == 1 copies.  lanes in [1, 256] and n % lanes == 0, else BASIC_ERR_INVALID. */
int basic_group_lanes_pack_dev(const int32_t *d_sym, const int32_t *d_idx, int batch, int64_t n, const int64_t *d_bases, int groups,
                               int lanes, int32_t *d_sym_out, int32_t *d_idx_out, void *hip_stream);
/* Skip coding (no reference counterpart; an opt-in format, INTEGRATION.md "Skip coding"): an element whose table row is below
 * skip_rows is not coded, and the decoder rebuilds it as symbol 0.  Both sides obtain the rows from the same index kernel on the
 * same prior, so the rule needs no side information.  keep(i) = d_idx[i] >= skip_rows.
 *
 * basic_skip_compact_dev: d_sym / d_idx are dense int32 [nstreams][per].  The outputs hold the kept elements of stream 0, then of
 * stream 1, and so on, back to back and each in its original order; d_seg int64 [nstreams + 1]: d_seg[s] = elements kept before
 * stream s, d_seg[nstreams] = the total -- what basic_rans_encode_batch_dev / basic_rans_decode_batch_dev take as they stand.
 * d_sym == NULL with d_sym_out == NULL: indexes and segments only (the decoder's call).  The outputs must hold nstreams * per
 * elements (everything may be kept), out of place.  skip_rows == 0 copies, d_seg[s] = s * per.
 *
 * basic_skip_expand_dev: the inverse.  The j-th kept element of stream s receives d_sym_compact[d_seg[s] + j], a skipped one 0;
 * d_idx_dense is the dense index array the compaction read.  The call RECOMPUTES the positions from d_idx_dense (a count and a
 * scan launch of its own): it needs no d_seg and nothing a compact call left in d_scratch, which may be any scratch of the size.
 *
 * Three launches each: per-chunk counts (a workgroup reads BASIC_SKIP_CHUNK elements of one stream, 16 bytes a lane where the
 * lane's four elements are 16-byte aligned and inside the stream, element by element otherwise), one workgroup's exclusive scan of
 * the counts in int64, and the scatter (ranks inside a chunk from wave ballots and an LDS sum over the waves).  No workgroup waits on
 * another and no atomic decides a position: the output is a function of the input alone.  Chunk c of stream s covers elements
 * [c * BASIC_SKIP_CHUNK, min(per, (c + 1) * BASIC_SKIP_CHUNK)); a stream has ceil(per / BASIC_SKIP_CHUNK) chunks.
 * d_scratch: BASIC_SKIP_SCRATCH_BYTES(nstreams, per) bytes of device memory, 8-byte aligned, private to the call until the stream
 * has passed it.  BASIC_ERR_INVALID, before any launch: a null pointer, nstreams < 1, per < 1, skip_rows < 0, d_sym without
 * d_sym_out or the reverse, a misaligned d_scratch, more than 2^30 chunks. */
#define BASIC_SKIP_CHUNK 1024
#define BASIC_SKIP_SCRATCH_BYTES(nstreams, per) \
    (8 * (size_t)(nstreams) * (((size_t)(per) + BASIC_SKIP_CHUNK - 1) / BASIC_SKIP_CHUNK))
int basic_skip_compact_dev(const int32_t *d_sym, const int32_t *d_idx, int nstreams, int64_t per, int skip_rows, void *d_scratch,
                           int32_t *d_sym_out, int32_t *d_idx_out, int64_t *d_seg, void *hip_stream);
int basic_skip_expand_dev(const int32_t *d_sym_compact, const int32_t *d_idx_dense, int nstreams, int64_t per, int skip_rows,
                          void *d_scratch, int32_t *d_sym_dense_out, void *hip_stream);
/* EntropyBottleneck path (compressai_coder.py:230-245): sym = round(z - median[c]),
 * idx = c, zhat = sym + median[c].  Layout [B][C][HW]. */
int basic_eb_quantize_index_dev(const float *d_z, const float *d_medians, int batch, int channels, int hw,
                                int32_t *d_symbols, int32_t *d_indexes, float *d_zhat, void *hip_stream);
int basic_eb_dequantize_dev(const int32_t *d_symbols, const float *d_medians, int batch, int channels,
                            int hw, float *d_zhat, void *hip_stream);
/* int32 symbols -> float32 (GaussianConditional.decompress/dequantize without means). */
int basic_i32_to_f32_dev(const int32_t *d_in, int64_t n, float *d_out, void *hip_stream);

/* Gaussian PGM coder (pgm_coder.py:735-821, torch_ans.py:279-282) evaluated on the element
 * list of ONE topo group.  Every image of the batch is an independent stream and shares the
 * list d_elems (int32 per-image element ids c*HW+p in coding order = ascending flat index,
 * pgm_coder.py:898-900).  params are "split_interleave" (channel 2c = mean, 2c+1 = scale)
 * in a [B][2C][HW] tensor; y / ybuf are [B][C][HW].  For element k of image b:
 *    idx = argmin_j |scale - table[j]| (first minimum),  mu = mean,
 *    sym = round_half_even(y - mu),  ybuf = sym + mu          (pgm_coder.py:927-941)
 * Outputs are dense per image: d_symbols/d_indexes[b*per_image + out_base + k]. */
int basic_pgm_gauss_encode_group_dev(const float *d_y, const float *d_params, int batch, int channels, int hw,
                                     const int32_t *d_elems, int64_t n_elems, const float *d_table,
                                     int table_len, int32_t *d_symbols, int32_t *d_indexes, int64_t per_image,
                                     int64_t out_base, float *d_ybuf, void *hip_stream);
/* Decoder half: indexes only (before rANS, pgm_coder.py:962-966) ... */
int basic_pgm_gauss_index_group_dev(const float *d_params, int batch, int channels, int hw,
                                    const int32_t *d_elems, int64_t n_elems, const float *d_table,
                                    int table_len, int32_t *d_indexes, int64_t per_image, int64_t out_base,
                                    void *hip_stream);
/* ... and reconstruction (after rANS, pgm_coder.py:973-978): ybuf = sym + mu. */
int basic_pgm_gauss_scatter_group_dev(const int32_t *d_symbols, const float *d_params, int batch, int channels,
                                      int hw, const int32_t *d_elems, int64_t n_elems, int64_t per_image,
                                      int64_t in_base, float *d_ybuf, void *hip_stream);

/* Rate estimate of the forward() pass ("prior_entropy", nats per image): d_nll[b] = -sum log(max(P(q), likelihood_bound)).
 *   interleaved_mean_scale == 0: CompressAI GaussianConditional likelihood (call site compressai_coder.py:352-375),
 *       zero mean, d_scales_or_params = scales [B][C][HW];
 *   interleaved_mean_scale == 1: PGM coder likelihood (pgm_coder.py:374-389), d_scales_or_params = [B][2C][HW] with
 *       channel 2c = mean, 2c+1 = scale.  d_q = the quantised latent [B][C][HW] (or, for the train-mode proxy, the latent
 *       plus uniform noise);
 *   interleaved_mean_scale == 2: the same parameters, likelihood of the ROUNDED RESIDUAL round(d_q - mean) under the zero-mean
 *       density (training_no_quantize_for_likelihood in eval mode, pgm_coder.py:376-387); d_q = the UNQUANTISED latent. */
int basic_gauss_nll_per_image_dev(const float *d_q, const float *d_scales_or_params, int batch, int channels, int hw,
                                  int interleaved_mean_scale, float scale_bound, float likelihood_bound, float *d_nll,
                                  void *hip_stream);
/* The interleaved_mean_scale == 0 mode under a quantiser step: d_q = the coded symbols round(y / step) as float32 [B][C][HW],
 * likelihood under s' = max(scale, scale_bound) / step[b] (the division of basic_gc_quantize_index_q_dev); d_steps float32
 * [n_steps] on the device, n_steps 1 or batch. */
int basic_gauss_nll_per_image_q_dev(const float *d_q, const float *d_scales, int batch, int channels, int hw, const float *d_steps,
                                    int n_steps, float scale_bound, float likelihood_bound, float *d_nll, void *hip_stream);
/* EntropyBottleneck likelihood (call site compressai_coder.py:203-228); d_coef float32 [C][58]: the pre-activated
 * 1-3-3-3-3-1 cumulative-logit network of every channel (softplus(matrix), bias, tanh(factor) per layer). */
int basic_eb_nll_per_image_dev(const float *d_zq, const float *d_coef, int batch, int channels, int hw,
                               float likelihood_bound, float *d_nll, void *hip_stream);

/* ======================================================================================
 * 5. Transforms: implicit-GEMM convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32) with fused
 *    bias + activation / (I)GDN epilogue.  Replaces the ATen calls behind
 *    nn/models/google.py:25-101, nn/layers/slimmable_layers.py:157-183,258-282.
 * ==================================================================================== */
typedef struct basic_conv_plan basic_conv_plan;

#define BASIC_ACT_NONE 0
#define BASIC_ACT_RELU 1
#define BASIC_ACT_LEAKY_RELU 2 /* slope 0.01 (torch default) */
#define BASIC_ACT_GDN 3        /* y = x * rsqrt(beta + gamma . x^2)   */
#define BASIC_ACT_IGDN 4       /* y = x * sqrt (beta + gamma . x^2)   */

/* Create a plan from host weights in PyTorch layout.
 *   transposed == 0: weight [cout][cin][k][k]  (nn.Conv2d),   out = floor((in+2p-k)/s)+1
 *   transposed == 1: weight [cin][cout][k][k]  (nn.ConvTranspose2d), out = (in-1)*s-2p+k+output_padding
 * bias may be NULL.  For GDN/IGDN, gamma [cout][cout] and beta [cout] are the EFFECTIVE
 * (already re-parametrised, non-negative) values.  cin_active/cout_active <= cin/cout select
 * the slimmable sub-network (weight slicing W[:co,:ci], slimmable_layers.py:142-170). */
int basic_conv_plan_create(const float *weight, const float *bias, int cin, int cout, int ksize, int stride,
                           int padding, int output_padding, int transposed, int activation,
                           const float *gamma, const float *beta, int cin_active, int cout_active,
                           basic_conv_plan **out);
int basic_conv_plan_out_hw(const basic_conv_plan *p, int in_h, int in_w, int *out_h, int *out_w);
/* Active (sliced) channel counts of the plan's input and output tensors. */
int basic_conv_plan_channels(const basic_conv_plan *p, int *cin_active, int *cout_active);
/* d_in: float32 [batch][cin_active][in_h][in_w]; d_out: float32 [batch][cout_active][out_h][out_w]. */
int basic_conv_forward_dev(const basic_conv_plan *p, const float *d_in, int batch, int in_h, int in_w,
                           float *d_out, void *hip_stream);
void basic_conv_plan_destroy(basic_conv_plan *p);
/* 2*MACs of one forward (conv + GDN), for roofline accounting. */
int64_t basic_conv_plan_flops(const basic_conv_plan *p, int batch, int in_h, int in_w);
/* Kernel launches one forward call makes for this input (sub-pixel phases of transposed convolutions, fused or not;
 * 32-channel slices count once: they share a launch). -1 on bad arguments. */
int basic_conv_plan_launches(const basic_conv_plan *p, int batch, int in_h, int in_w);

/* ======================================================================================
 * 6. Topo-group masked convolution (TopoGroupDynamicMaskConv2d.forward,
 *    nn/layers/masked_conv.py:102-228) evaluated ONLY at a list of positions -- the positions
 *    of the topo group being coded -- instead of the full map the reference recomputes for
 *    every group (pgm_coder.py:922-924,958-961).  One operator serves the 5x5 context conv
 *    and the 1x1 "param merger" layers (pgm_coder.py:1215-1239, masked_conv.py:262-300):
 *      y[b,co,p] = bias[co] + sum_{ci,tap} W[co,ci,tap] * x[b,ci,p+tap]
 *                    * [ topo_in[g_in(ci), p+tap]  (< | <=)  topo_out[g_out(co), p] ]
 * ==================================================================================== */
typedef struct basic_mconv_plan basic_mconv_plan;
/* weight [cout][cin][k][k] (k in {1,3,5}, padding k/2), bias [cout] or NULL.
 * in_groups/out_groups: contiguous channel groups of x / y; allow_same_topogroup selects <=. */
int basic_mconv_plan_create(const float *weight, const float *bias, int cin, int cout, int ksize,
                            int in_groups, int out_groups, int allow_same_topogroup, int activation,
                            basic_mconv_plan **out);
/* d_x [B][cin][H][W]; d_topo_in int32 [in_groups][H][W]; d_topo_out int32 [out_groups][H][W];
 * d_pos int32 [n_pos] flat ids b*H*W + y*W + x.  Writes channels
 * [out_channel_offset, out_channel_offset+cout) of d_y [B][out_channels_total][H][W] at the
 * listed positions only. */
int basic_mconv_forward_pos_dev(const basic_mconv_plan *p, const float *d_x, const int32_t *d_topo_in,
                                const int32_t *d_topo_out, int batch, int h, int w, const int32_t *d_pos,
                                int64_t n_pos, float *d_y, int out_channels_total, int out_channel_offset,
                                void *hip_stream);
/* The same operator inside the group-sequential coding loop (pgm_coder.py:921-941 / :958-978), where d_y persists
 * across the steps of one encode / decode: only (output group, position) pairs whose topo id equals `step` are
 * evaluated -- plus groups without a topo id (-1) at the first step that visits the position (d_first_step int32
 * [H][W] = min over channel groups of the topo ids).  Everything else in d_y is either already exact (earlier steps;
 * the mask makes a value depend only on elements coded before its own step) or not needed yet.  The reference
 * recomputes the full map at every step instead. */
int basic_mconv_forward_step_dev(const basic_mconv_plan *p, const float *d_x, const int32_t *d_topo_in,
                                 const int32_t *d_topo_out, int batch, int h, int w, const int32_t *d_pos,
                                 int64_t n_pos, float *d_y, int out_channels_total, int out_channel_offset,
                                 int step, const int32_t *d_first_step, void *hip_stream);
/* Everything at once: use_step != 0 = the coding-loop variant above; d_in_perm / d_out_perm (int32 [H*W] or NULL) permute
 * the positions inside the planes of x / y -- element (b, c, p) at (b * C + c) * H*W + perm[p] -- for buffers that are
 * PRIVATE to a chain of 1x1 layers (the merger's hidden activations): with a coding step's positions contiguous its gathers
 * and stores cover whole cache lines.  d_in_perm needs a 1x1 layer.  Values are unaffected. */
int basic_mconv_forward_ex_dev(const basic_mconv_plan *p, const float *d_x, const int32_t *d_topo_in,
                               const int32_t *d_topo_out, int batch, int h, int w, const int32_t *d_pos, int64_t n_pos,
                               float *d_y, int out_channels_total, int out_channel_offset, int use_step, int step,
                               const int32_t *d_first_step, const int32_t *d_in_perm, const int32_t *d_out_perm,
                               void *hip_stream);
/* Which kernel serves a launch (csrc/mconv.hip: all of them sum in one canonical order, so the choice is a matter of speed). */
#define BASIC_MCONV_KERNEL_NONE (-1) /* no launch yet, or nothing to launch (n_pos == 0) */
#define BASIC_MCONV_KERNEL_GATHER 0
#define BASIC_MCONV_KERNEL_BLOCK 1
#define BASIC_MCONV_KERNEL_DMA 2
/* *kernel = what the last forward call on this plan launched; BASIC_MCONV_KERNEL_NONE before any launch. */
int basic_mconv_last_kernel(const basic_mconv_plan *p, int *kernel);
/* What a forward call of such a layer would launch for n_pos listed positions of `batch` h x w maps, without a plan or a
 * device: one host function in csrc/mconv.hip answers this and picks the kernel of every forward call.  It honours the
 * environment variable BASIC_MCONV_KERNEL = gather | block | dma; a forced kernel that does not serve the launch (block: more
 * than 4096 (tile, block) units; dma: a layer without 64-channel input groups, 128-row output groups and at most 64 (tap,
 * input group) slabs) leaves it to the gather kernel. */
int basic_mconv_choose(int cin, int cout, int ksize, int in_groups, int out_groups, int batch, int h, int w, int64_t n_pos,
                       int *kernel);
void basic_mconv_plan_destroy(basic_mconv_plan *p);

/* ======================================================================================
 * 7. Distortion metric: per-image PSNR pieces (benchmark/metrics/pytorch_distortion.py:12-15):
 *    d_mse[b] = mean((a-b)^2) over C*H*W in float32 accumulate-by-tree.
 * ==================================================================================== */
int basic_mse_per_image_dev(const float *d_a, const float *d_b, int batch, int64_t elems_per_image,
                            float *d_mse, void *hip_stream);
/* MS-SSIM per image: pytorch_msssim.ms_ssim(x_hat, x, data_range, size_average) as consumed at
 * cbench/benchmark/metrics/pytorch_distortion.py:8,17-18 and cbench/modules/entropy_coder/latent_graph.py:14,92-96, with that
 * package's defaults (11-tap Gaussian window of sigma 1.5 without padding, K = (0.01, 0.03), five scales with weights
 * (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)).  PARITY-UNPINNED: the package is not available; the kernels (csrc/msssim.hip)
 * evaluate what benchmark/ms_ssim.py states.  min(h, w) must exceed 160 (four halvings must leave room for the window).
 * Bytes of device workspace a call for this shape needs (pooled pyramids of both images, one partial sum per map tile):
 * pure host arithmetic, no device needed; does not decrease in any argument; -1 on bad arguments. */
int64_t basic_msssim_workspace_bytes(int batch, int channels, int h, int w);
/* d_x, d_y: float32 [batch][channels][h][w].  d_msssim[b] = mean over channels of the weighted product of the five terms;
 * d_terms (may be NULL): float32 [batch][channels][5], the terms before the weights: relu(mean cs) of scales 0-3 and
 * relu(mean ssim) of scale 4.  Ten launches on hip_stream; nothing is allocated and nothing synchronised inside the call,
 * and no float atomics: the value of an image is bit-for-bit the same at any batch size, batch position and stream.
 * d_workspace: at least workspace_bytes >= basic_msssim_workspace_bytes of device memory, float-aligned, private to the call
 * until the stream has passed it.  BASIC_ERR_INVALID for a null pointer, a side <= 160 or a workspace that is too small. */
int basic_msssim_per_image_dev(const float *d_x, const float *d_y, int batch, int channels, int h, int w, float data_range,
                               void *d_workspace, int64_t workspace_bytes, float *d_msssim, float *d_terms, void *hip_stream);

/* ======================================================================================
 * 8. Fused image entry points of the two hyperprior latent graphs (SURVEY 8b "basic_encode_image / decode_image"): the scale
 *    hyperprior (h_s ends in y_channels planes, the scales; y coded as round(y)) and the mean-scale hyperprior (h_s ends in
 *    2 * y_channels planes, scales [0, M) then means [M, 2 M); y coded as round(y - mean) with the basic_gc_*_ms_dev entry points of
 *    section 4, both halves read where h_s left them).  basic_hp_session_create tells them apart by h_s's last plan; every setter,
 *    the z path, lane streams and the wire format are the same for both.
 *    ONE call runs what GeneralCodec.compress / decompress run for that graph
 *      compress   general_codec.py:44-89 -> LatentGraphicalANSEntropyCoder.encode latent_graph.py:1232-1264
 *                 x -> g_a -> y -> h_a -> z ; EntropyBottleneck coder (compressai_coder.py:230-236) ; h_s ;
 *                 GaussianConditional coder (:377-385) ; merge_bytes([z body, y body], num_segments=2)
 *      decompress general_codec.py:91-130 -> .decode latent_graph.py:1266-1295 ; g_s
 *    with the same kernels in the same order as the module-by-module path, so the bytes are identical; the host
 *    side of a call is ~60 kernel launches from C++ instead of a Python interpreter walking the graph.
 *    A session BORROWS the layer plans and table sets (they must outlive it), owns its device workspace and pinned
 *    staging buffers, and serves one call at a time (one session per host thread / HIP stream).
 *    Wire format: [u32 native-endian len(z body)] [z body] [y body]; a body is write_body's ">III" (h, w, n) followed by
 *    ">I" length + rANS words per image (compressai_coder.py:63-84).
 * ==================================================================================== */
typedef struct basic_hp_session basic_hp_session;
/* g_a / h_a / h_s / g_s: the fused layer plans of each transform in execution order.  eb_medians: float32
 * [z_channels] (host).  scale_table: float32 [n_scales] (host), scale_bound = GaussianConditional's lower bound. */
int basic_hp_session_create(const basic_conv_plan *const *g_a, int n_g_a, const basic_conv_plan *const *h_a, int n_h_a,
                            const basic_conv_plan *const *h_s, int n_h_s, const basic_conv_plan *const *g_s, int n_g_s,
                            const float *eb_medians, int z_channels, const basic_rans_tables *z_tables,
                            const float *scale_table, int n_scales, float scale_bound,
                            const basic_rans_tables *y_tables, basic_hp_session **out);
/* Upper bound of basic_hp_encode_images' output for this input shape (always sufficient). */
int64_t basic_hp_encode_bound(const basic_hp_session *s, int batch, int h, int w);
/* x: float32 [batch][cin][h][w], on the device (x_on_host == 0) or in host memory (x_on_host != 0: uploaded inside the
 * call on hip_stream -- asynchronously when the memory is page-locked -- as GeneralCodec.compress does,
 * general_codec.py:46-47).  Returns with the bytes complete in `out` (the stream has been synchronised). */
int basic_hp_encode_images(basic_hp_session *s, const float *x, int x_on_host, int batch, int h, int w, uint8_t *out,
                           int64_t out_capacity, int64_t *out_len, void *hip_stream);
/* With out == NULL basic_hp_encode_images only reports the size in *out_len and keeps the encoded batch in the session
 * (page-locked host memory); this call frames it into caller memory (any number of times, until the next encode). */
int basic_hp_encode_result(basic_hp_session *s, uint8_t *out, int64_t out_capacity, int64_t *out_len);
/* Shape of the reconstruction a stream decodes to (from its headers only). */
int basic_hp_decoded_shape(const basic_hp_session *s, const uint8_t *data, int64_t len, int *batch, int *channels, int *h,
                           int *w);
/* d_xhat: float32 [batch][channels][h][w] on the device (the un-clamped output of g_s).  The work is ENQUEUED on
 * hip_stream; the call returns once the stream words have left `data` (no final synchronisation). */
int basic_hp_decode_images(basic_hp_session *s, const uint8_t *data, int64_t len, float *d_xhat,
                           int64_t xhat_capacity_floats, void *hip_stream);
/* Lane streams of the y latent (INTEGRATION.md "Lane streams"): the y path codes batch * lanes rANS streams of ny / lanes
 * symbols -- stream b * lanes + k holds symbols [k ny / lanes, (k + 1) ny / lanes) of image b in (c, h, w) order -- and the y
 * body holds batch * lanes streams; the z body is untouched.  lanes in [1, 256]; 1 (the default) is the reference's format.
 * A call whose ny is no multiple of lanes, or a stream whose y body does not hold lanes streams per z stream, fails with
 * BASIC_ERR_INVALID.  Configuration of the session like its tables: not written into the stream. */
int basic_hp_session_set_stream_lanes(basic_hp_session *s, int lanes);
/* Quantiser step of the y latent (section 4; INTEGRATION.md "Quantiser step"): host_steps = n float32 in host memory, one for
 * every image of the calls that follow (n == their batch) or one for all (n == 1); n == 0 clears it, and the session launches
 * exactly what it launched before.  Every step must be finite and in [BASIC_QSTEP_MIN, BASIC_QSTEP_MAX], else
 * BASIC_ERR_INVALID and the session keeps what it had.  With steps set, basic_hp_encode_images[_u8] and
 * basic_hp_decode_images[_u8] copy them to the device on the call's stream and take basic_gc_quantize_index_q_dev /
 * basic_gc_dequantize_q_dev on the y path; z stays at step 1, lane streams keep their meaning, and the two bodies keep their
 * format.  A call whose batch is neither n nor broadcast from n == 1 fails with BASIC_ERR_INVALID before anything is launched.
 * The steps are NOT written into the stream: the container that carries them is the caller's (codecs/qstep.py). */
int basic_hp_session_set_qsteps(basic_hp_session *s, const float *host_steps, int n);
/* Rate targets (section 4, "Rate control"): host_budget_bytes = n int64 byte budgets, one per image of the calls that follow or one
 * for all (n == 1); n == 0 clears them.  A budget covers an image's payload: its z stream plus its y stream(s).  host_cand: n_cand
 * in [2, 32] float32 candidate steps, strictly ascending, inside [BASIC_QSTEP_MIN, BASIC_QSTEP_MAX]; passes in [1, 3].  With targets
 * set, basic_hp_encode_images[_u8] runs curve -> select -> (refine -> curve -> select) x (passes - 1) in front of the y quantiser, on
 * the call's stream, the z streams' word counts as extra_words, and the y path reads the steps the select kernel wrote: the bytes
 * are those of the same call under basic_hp_session_set_qsteps with these steps.  No host synchronisation is added.  Refused while
 * quantiser steps are set, as basic_hp_session_set_qsteps is while targets are: one way to state the step at a time. */
int basic_hp_session_set_rate_targets(basic_hp_session *s, const int64_t *host_budget_bytes, int n, const float *host_cand, int n_cand,
                                      int passes);
/* The last rate-controlled encode call's choices, n = its batch: the steps, the predicted payload bytes and the select kernel's
 * d_choice word (BASIC_RATE_NO_FIT set: nothing fitted, the largest step was taken).  Any of the three may be NULL. */
int basic_hp_session_rate_result(const basic_hp_session *s, float *steps, int64_t *pred_bytes, int32_t *flags, int n);
/* Skip coding of the y latent (section 4, "Skip coding"): rows in [0, n_scales]; 0 (the default) is the format without it, and the
 * session launches exactly what it launched before.  With rows > 0 the encoder compacts the y symbols and indexes behind the
 * quantise launch (basic_skip_compact_dev) and codes the compacted streams; the decoder compacts the indexes, decodes, expands
 * (basic_skip_expand_dev) and de-quantises with the unchanged kernels, so a skipped element is rebuilt as symbol 0: yhat = 0, or the
 * mean.  Quantiser steps (the rows are then those of sigma / step), lane streams (every lane's run is shortened on its own), the
 * mean-scale graph and the uint8 entry points keep their meaning; the body's format is unchanged, its streams are shorter.  Refused
 * with BASIC_ERR_INVALID while rate targets are set, as basic_hp_session_set_rate_targets is while rows > 0: the rate curve counts
 * symbols that would not be coded.  Not written into the stream: the container that carries it is the caller's (utils/skip.py). */
int basic_hp_session_set_skip_rows(basic_hp_session *s, int rows);
/* Wavefronts (image streams) per workgroup of this session's rANS launches: 1, 2, 4, 8 or 16 (0 = library default). */
int basic_hp_session_set_rans_waves(basic_hp_session *s, int waves_per_block);
/* Opt this session into the process-wide "transform token": the MFMA-heavy phases (compress: everything up to the y
 * rANS encoder; decompress: g_s) of all such sessions then run one after another in GPU time, in host enqueue order,
 * through stream-wait events -- so that with several sessions on several HIP streams one session's rANS chains always
 * run beside another's transforms instead of all sessions falling into lock-step.  enable = 1: one phase at a time (full
 * batches fill the chip on their own); 2: two at a time (small batches, whose launches leave compute units idle); 0: off.
 * The order is kept per device.  No effect on results. */
int basic_hp_session_set_transform_token(basic_hp_session *s, int enable);
void basic_hp_session_destroy(basic_hp_session *s);

/* ======================================================================================
 * 8b. 8-bit images (csrc/image.hip): uint8 in, uint8 out, converted on the device in front of the unchanged first layer
 *    and behind the unchanged last one.  Replaces the host-side ingest of
 *    cbench/data/datasets/torchvision_datasets.py:80-88 (PIL -> ToTensor: permute to CHW, float32, divide by 255) and the
 *    clamp / scale / round / cast a caller runs on a reconstruction before it writes a picture.
 *      uint8 -> float32:  f = float32(u) / float32(255), correctly rounded (a 256-entry table of host-computed quotients;
 *                         a reciprocal multiply is NOT equal to it for all 256 inputs).
 *      float32 -> uint8:  q = uint8(rint(min(max(x, 0), 1) * 255.0f)), rint = round-half-to-even, one fp32 multiply, NaN -> 0:
 *                         torch.nan_to_num(x, nan=0.0).clamp(0, 1).mul(255).round().to(torch.uint8) evaluated on the CPU.
 *    The float side is always [batch][channels][h][w]; the uint8 side is BASIC_IMAGE_CHW, [batch][channels][h][w], or
 *    BASIC_IMAGE_HWC, [batch][h][w][channels] (what every image decoder delivers).  Element offsets are 64-bit.
 *    Any channels, h, w >= 1 and any byte alignment of the uint8 pointer; the float pointer must be float-aligned.
 *    A call takes the wide path (one dword of four samples per lane against 16-byte float accesses) when the uint8
 *    pointer is 4-byte and the float pointer 16-byte aligned and, for BASIC_IMAGE_HWC, channels is 3 or 4 and h * w a
 *    multiple of 4 (a lane then owns four consecutive pixels: `channels` dwords against one 16-byte vector per plane);
 *    the last batch * channels * h * w % 4 samples of a BASIC_IMAGE_CHW call and every other call go sample by sample.
 *    Both paths give the same values.  BASIC_ERR_INVALID, before any launch, for a non-positive dimension, a null
 *    pointer, an unknown layout, a misaligned float pointer or more than 2^40 samples.
 * ==================================================================================== */
#define BASIC_IMAGE_CHW 0
#define BASIC_IMAGE_HWC 1
/* Ingest (torchvision_datasets.py:80-88 on the device): d_src uint8 in `layout`, d_dst float32 [batch][channels][h][w]. */
int basic_image_u8_to_f32_dev(const uint8_t *d_src, int layout, int batch, int channels, int h, int w,
                              float *d_dst, void *hip_stream);
/* The way back (the caller's x.clamp(0, 1).mul(255).round().byte()): d_src float32 [batch][channels][h][w], d_dst uint8 in
 * `layout`. */
int basic_image_f32_to_u8_dev(const float *d_src, int batch, int channels, int h, int w, int layout,
                              uint8_t *d_dst, void *hip_stream);
/* The distortion of an 8-bit picture, exactly: d_sse[b][c] = sum over (y, x) of (a - b)^2 as an integer (PSNR of the batch
 * or of an image = 10 log10(255^2 * samples / sum of its d_sse), in float64 on the host).  d_a and d_b are uint8 batches of
 * one shape, EACH in its own layout (a decoded PNG is HWC, a reconstruction either).  Integer arithmetic only -- 32-bit sums
 * of at most 16 squares, 64-bit from there on -- and the workgroups meet in 64-bit integer atomic adds, one per workgroup and
 * destination, which commute: the result is the same at any batch, layout, alignment, launch shape and arrival order.  The
 * call clears d_sse on hip_stream itself (one memset node in front of the one launch) and writes every element of it;
 * nothing is allocated, nothing synchronised.  Any channels, h, w >= 1 and any byte alignment of either uint8 pointer.  With
 * both pointers 4-byte aligned a lane reads one dword of four samples per operand: two BASIC_IMAGE_CHW operands (or one
 * channel) by planes -- the up to three samples between a plane's ends and its whole dwords, where h * w % 4 != 0 puts two
 * channels or two images into one dword, are added one by one --, and, with an HWC operand, channels 3 or 4 and h * w a
 * multiple of 4, four consecutive pixels per lane (`channels` dwords of an HWC operand, one dword per plane of a CHW one).
 * Every other call goes sample by sample.  All paths give the same integers.  BASIC_ERR_INVALID, before any launch, for a
 * non-positive dimension, a null pointer, an unknown layout, a d_sse that is not 8-byte aligned or more than 2^40 samples. */
int basic_image_sse_u8_dev(const uint8_t *d_a, int layout_a, const uint8_t *d_b, int layout_b,
                           int batch, int channels, int h, int w,
                           uint64_t *d_sse /* [batch][channels] */, void *hip_stream);
/* basic_hp_encode_images for a uint8 batch in `layout` (channels = the first layer's input channels), on the device
 * (x_on_host == 0) or in host memory: a host batch is copied as uint8 -- a quarter of the float bytes -- into a staging
 * buffer of the session on its copy stream and converted on hip_stream into the buffer the first layer reads; from there
 * on the call IS basic_hp_encode_images (same bytes, same basic_hp_encode_result, same lane settings).  The caller may
 * change hip_stream between calls. */
int basic_hp_encode_images_u8(basic_hp_session *s, const uint8_t *x, int x_on_host, int layout, int batch, int h, int w,
                              uint8_t *out, int64_t out_capacity, int64_t *out_len, void *hip_stream);
/* basic_hp_decode_images into a float buffer of the session, converted on hip_stream into xhat: uint8 in `layout`, on the
 * device (xhat_on_host == 0: enqueued, as basic_hp_decode_images) or in host memory (converted into a device staging
 * buffer and copied; the call returns with the picture complete in xhat).  xhat_capacity_bytes smaller than the
 * basic_hp_decoded_shape of the stream: BASIC_ERR_INVALID, nothing launched. */
int basic_hp_decode_images_u8(basic_hp_session *s, const uint8_t *data, int64_t len, int layout,
                              uint8_t *xhat, int xhat_on_host, int64_t xhat_capacity_bytes, void *hip_stream);

/* ======================================================================================
 * 8c. Tiles of one 8-bit picture (csrc/image.hip): a picture too large for one pass of the transforms, or one that is to
 *    be read in parts, is coded as independent tiles.  The first two entries are the first and the last step of that:
 *    they cut a batch of float tiles out of ONE uint8 picture, and paste a batch of reconstructed tiles back into one,
 *    each in one memory pass (instead of one strided copy per tile and a conversion pass over the batch).  Tiles that
 *    OVERLAP, so that the seams between them can be cross-faded, have two entries of their own further down: a cut that
 *    accepts them, and the blend that writes the picture from all their reconstructions.
 *    A tile group is a regular grid of equally sized tiles inside the picture: tile (i, j), i < ny, j < nx, has its
 *    origin at (y0 + i * step_y, x0 + j * step_x), is th x tw, and has index i * nx + j.  The picture is uint8,
 *    [channels][img_h][img_w] (BASIC_IMAGE_CHW) or [img_h][img_w][channels] (BASIC_IMAGE_HWC); the float side is always
 *    [ny * nx][channels][rows][cols].
 *    Values: exactly those of section 8b, from the same device code -- in, the 256-entry table of correctly rounded
 *    u / 255; out, uint8(rint(min(max(x, 0), 1) * 255.0f)), NaN -> 0.
 *    Element offsets are 64-bit.  Any channels, th, tw >= 1 and any byte alignment of the uint8 pointer; the float
 *    pointer must be float-aligned.  The paste writes only bytes inside its tiles: everything else in d_img keeps its
 *    value.  Nothing is allocated, nothing synchronised; each call is ONE launch on hip_stream.
 *    Wide path: a lane owns four consecutive samples of one tile row, one dword of uint8 against one 16-byte float
 *    access; with BASIC_IMAGE_HWC and channels 3 or 4 it owns `channels` dwords (four pixels) against one vector per
 *    plane.  Taken when the uint8 base is 4-byte and the float base 16-byte aligned, img_w, x0, step_x, tw (and sw for
 *    the paste) are multiples of 4 and, with BASIC_IMAGE_HWC and more than one channel, channels is 3 or 4 (one channel:
 *    the layouts coincide).  Every other call goes sample by sample.  Both paths give the same values.
 *    BASIC_ERR_INVALID with a message, before any launch, for a null pointer, an unknown layout, a non-positive
 *    dimension or step, a negative origin, a step smaller than the tile (overlapping tiles), a last tile that leaves the
 *    picture (y0 + (ny - 1) * step_y + th > img_h, likewise in x), sh < th or sw < tw, a misaligned float pointer, or
 *    more than 2^40 samples on the float side.
 * ==================================================================================== */
/* Cut + ingest: d_img uint8, one picture in `layout`; d_dst float32 [ny * nx][channels][th][tw]. */
int basic_image_tiles_u8_to_f32_dev(const uint8_t *d_img, int layout, int channels, int img_h, int img_w,
                                    int y0, int x0, int step_y, int step_x, int ny, int nx, int th, int tw,
                                    float *d_dst, void *hip_stream);
/* Convert + crop + paste: d_src float32 [ny * nx][channels][sh][sw] with sh >= th, sw >= tw (a synthesis transform
 * returns its own multiple of 64); the top-left th x tw of every tile goes to its place in d_img. */
int basic_image_tiles_f32_to_u8_dev(const float *d_src, int sh, int sw, int channels,
                                    int y0, int x0, int step_y, int step_x, int ny, int nx, int th, int tw,
                                    uint8_t *d_img, int layout, int img_h, int img_w, void *hip_stream);
/* The cut for OVERLAPPED tiles: basic_image_tiles_u8_to_f32_dev without the refusal of a step smaller than the tile
 * (step_y, step_x >= 1 is all that is asked; the tiles are only read, so they may share samples).  The same kernels, the
 * same values, the same wide / scalar rule and the same basic_image_tiles_last_path report. */
int basic_image_tiles_overlap_u8_to_f32_dev(const uint8_t *d_img, int layout, int channels, int img_h, int img_w,
                                            int y0, int x0, int step_y, int step_x, int ny, int nx, int th, int tw,
                                            float *d_dst, void *hip_stream);
/* Blend: the way back for overlapped tiles.  The grid is that of a whole picture (cbench_basic_amd/utils/tiling.py):
 * steps sy = th - oy, sx = tw - ox with 0 <= 2 oy <= th, 0 <= 2 ox <= tw; rows = max(1, ceil((img_h - oy) / sy)), cols
 * likewise; tile (i, j) has its origin at (i * sy, j * sx) and is th x tw, cut off at the picture's edge.  Along an axis
 * the samples [(i + 1) * s, (i + 1) * s + o) are covered by tiles i and i + 1, every other sample by one tile.
 * ONE launch writes the rectangle [ry0, ry0 + rh) x [rx0, rx0 + rw) of the picture, as a picture of its own --
 * [channels][rh][rw] (BASIC_IMAGE_CHW) or [rh][rw][channels] (BASIC_IMAGE_HWC), uint8 (BASIC_PIXEL_U8) or float32
 * (BASIC_PIXEL_F32) -- from the reconstructions of the tiles that cover it.  It is a gather: d_table, in DEVICE memory, has
 * one basic_tile_source per tile in row-major order; entry i * cols + j describes the float32 [channels][sh][sw]
 * reconstruction of tile (i, j), sh and sw at least the tile's own height and width (the caller's duty: the table cannot
 * be read from the host), wherever the decoder left it.  Entries of one table may differ in sh x sw.  No staging copy,
 * no accumulation buffer, no read of the output.
 * Values.  ramp[d] = (float)((2 * d + 1) / (2.0 * o)), d = 0 .. o - 1: a double division rounded once to fp32.
 * lerp(a, b, w) = a + w * (b - a): one fp32 subtract, one multiply, one add, each rounded, never a fused multiply-add.
 * A sample at distance d into the band of tiles i and i + 1 of one axis is lerp(a, b, ramp[d]), a from tile i, b from
 * tile i + 1.  In a band of both axes: top = lerp(r[i][j], r[i][j + 1], wx), bottom = lerp(r[i + 1][j], r[i + 1][j + 1],
 * wx), v = lerp(top, bottom, wy).  In no band: its tile's value.  The float output is v, the uint8 output section 8b's
 * uint8(rint(min(max(v, 0), 1) * 255.0f)), NaN -> 0, from the same device code.  So: where the covering tiles agree (and
 * are finite) the result is that value; with overlap 0 it is the paste; and a sample's value depends on the tiles that
 * cover it alone, not on the other entries, the chunks they came from or the launch shape.
 * A null src marks a tile that was not decoded.  The kernel never dereferences one: the output samples that need that
 * tile keep the value they had, every other sample of the rectangle is written.
 * Wide path: a lane owns four consecutive output samples of one row (one plane; with BASIC_IMAGE_HWC and channels 3 or 4,
 * four pixels of all channels) and reads each source with one 16-byte load where that source's address allows, four
 * 4-byte loads otherwise.  Taken when the output base is 4-byte (uint8) or 16-byte (float32) aligned, rx0, rw, sx and ox
 * are multiples of 4 -- the four samples then share their tiles and their band -- and, with BASIC_IMAGE_HWC and more than
 * one channel, channels is 3 or 4.  Every other call goes sample by sample.  Both paths give the same values;
 * basic_image_tiles_last_path reports the one taken.
 * Element offsets are 64-bit; one launch on hip_stream, nothing allocated, nothing synchronised.  BASIC_ERR_INVALID with
 * a message, before any launch, for a null pointer, an unknown layout or out_kind, a non-positive size, a negative
 * overlap or one above half a tile, a rectangle that leaves the picture, a float32 output that is not float-aligned, or
 * more than 2^40 output samples. */
#define BASIC_PIXEL_U8 0
#define BASIC_PIXEL_F32 1
typedef struct basic_tile_source {
    const float *src; /* [channels][sh][sw] in device memory, or NULL: not decoded */
    int32_t sh, sw;
} basic_tile_source;
int basic_image_tiles_blend_dev(const basic_tile_source *d_table /* [rows * cols], device memory */,
                                int img_h, int img_w, int th, int tw, int oy, int ox, int channels,
                                int ry0, int rx0, int rh, int rw, void *d_out, int out_kind, int layout,
                                void *hip_stream);
/* The path the calling thread's last tiles call took: 0 scalar, 1 wide; -1 before any (as basic_rans_last_launch: written
 * where the kernel is chosen, read by tests). */
int basic_image_tiles_last_path(int *path);

/* ======================================================================================
 * 8d. Tiles of MANY 8-bit pictures (csrc/image.hip): the cut and the paste of section 8c driven by a table with one row per
 *    tile, so that one launch reads or writes tiles of any number of pictures.  Pictures of different sizes share no batch
 *    shape, but their tiles do: a caller pools the th x tw tiles of a whole set of pictures into one float batch and codes
 *    that (cbench_basic_amd/utils/tiling.py: pool_tiles).
 *    Row t of the table says where tile t of the float batch lies: the picture (device memory, uint8, [channels][img_h][img_w]
 *    for BASIC_IMAGE_CHW or [img_h][img_w][channels] for BASIC_IMAGE_HWC), its size, and the tile's origin (y0, x0) in it.
 *    Rows of one table may differ in picture, size and layout; rows may name the same picture again, and rows of a gather may
 *    overlap (overlapped tiles need no entry of their own here).  Rectangles of ONE SCATTER that intersect in one picture are
 *    the caller's duty: which tile's bytes such a sample ends up with is not defined.  The scatter writes only bytes inside
 *    its tiles.
 *    The table is passed in HOST memory, so that every row is checked before anything runs on the GPU; the entry then copies
 *    it to the caller's device workspace d_table_ws (n rows, 8-byte aligned) on hip_stream and waits for that copy -- and,
 *    with it, for what hip_stream held before -- so the host table may be reused when the call returns.  The launch itself
 *    is enqueued, not awaited: d_table_ws, the pictures and the batch stay untouched until it has run.  One launch per call,
 *    nothing allocated, 64-bit element offsets.
 *    Values: exactly those of sections 8b / 8c, from the same device code.  A gathered tile equals, bit for bit, what
 *    basic_image_tiles_u8_to_f32_dev gives for that picture and origin; a scattered tile what
 *    basic_image_tiles_f32_to_u8_dev writes.
 *    Wide path (the rule of 8c, decided on the host): a lane owns four consecutive samples of a tile row -- with
 *    BASIC_IMAGE_HWC and 3 or 4 channels four pixels -- when the float base is 16-byte aligned, tw (and sw for the scatter)
 *    is a multiple of 4 and EVERY row has a 4-byte aligned picture, img_w and x0 multiples of 4 and, where its layout is
 *    BASIC_IMAGE_HWC with more than one channel, 3 or 4 channels.  Otherwise the whole launch goes sample by sample.
 *    basic_image_tiles_last_path reports the path.  A workgroup reads a tile's row once.
 *    BASIC_ERR_INVALID with a message, before any copy or launch, for a null pointer (table, workspace, batch, or a row's
 *    picture), n < 1, a non-positive size, an unknown layout, a negative origin, y0 + th > img_h or x0 + tw > img_w in any
 *    row, sh < th or sw < tw, a misaligned float pointer or workspace, or more than 2^40 float samples.
 * ==================================================================================== */
typedef struct basic_tile_ref {
    void   *img;            /* uint8 picture in device memory */
    int32_t img_h, img_w;   /* its size */
    int32_t y0, x0;         /* the tile's origin in it */
    int32_t layout;         /* BASIC_IMAGE_CHW / BASIC_IMAGE_HWC, per entry */
} basic_tile_ref;
/* Cut + ingest: tile t of d_dst, float32 [n][channels][th][tw], is the th x tw rectangle at (y0, x0) of table[t].img. */
int basic_image_tiles_gather_u8_to_f32_dev(const basic_tile_ref *table /* HOST, n entries */, int n, int channels,
                                           int th, int tw, basic_tile_ref *d_table_ws /* device, n entries */,
                                           float *d_dst, void *hip_stream);
/* Convert + crop + paste: the top-left th x tw of tile t of d_src, float32 [n][channels][sh][sw], goes to (y0, x0) of
 * table[t].img. */
int basic_image_tiles_scatter_f32_to_u8_dev(const float *d_src, int sh, int sw, int channels, int th, int tw,
                                            const basic_tile_ref *table /* HOST */, int n, basic_tile_ref *d_table_ws,
                                            void *hip_stream);
/* Edge-padded tiles: the two entries above for tiles of ph x pw that may leave their picture at the bottom and right (a tile
 * coded at its size rounded up: cbench_basic_amd/utils/tiling.py, pad_to).  Same signatures, same host-checked table, same
 * staging, one launch each, nothing allocated.  The origin of every row lies inside its picture: 0 <= y0 < img_h,
 * 0 <= x0 < img_w.
 *   gather_pad : d_dst[t][c][r][q] = picture[c][min(y0 + r, img_h - 1)][min(x0 + q, img_w - 1)] / 255 for r < ph, q < pw: the
 *                picture's last row and column replicated into the part of the tile outside it.  A table in which no tile
 *                leaves its picture gives, bit for bit, basic_image_tiles_gather_u8_to_f32_dev's output.
 *   scatter_clip: writes the part of each tile's top-left ph x pw that lies inside its picture, and no other byte.
 * Wide path: today's rule (float base 16-byte aligned, pw -- and sw -- multiples of 4, every row a 4-byte aligned picture with
 * img_w and x0 multiples of 4, interleaved rows only with 3 or 4 channels).  Under it a run of four samples is wholly inside
 * or wholly outside a picture row: an outside run of the gather is the row's last pixel in all four places (byte 3 of the
 * row's last dword; pixel 3 of its last four interleaved pixels), rows at or beyond img_h read row img_h - 1, and the scatter
 * skips outside runs and rows.  Otherwise the launch goes sample by sample and clamps, or tests, each sample.
 * basic_image_tiles_last_path reports the path.
 * BASIC_ERR_INVALID with a message, before any copy or launch: the refusals of the two entries above, with "the tile leaves
 * the picture" replaced by "the tile's origin leaves the picture" (y0 >= img_h or x0 >= img_w in any row). */
int basic_image_tiles_gather_pad_u8_to_f32_dev(const basic_tile_ref *table /* HOST, n entries */, int n, int channels,
                                               int ph, int pw, basic_tile_ref *d_table_ws /* device, n entries */,
                                               float *d_dst, void *hip_stream);
int basic_image_tiles_scatter_clip_f32_to_u8_dev(const float *d_src, int sh, int sw, int channels, int ph, int pw,
                                                 const basic_tile_ref *table /* HOST */, int n, basic_tile_ref *d_table_ws,
                                                 void *hip_stream);

/* ======================================================================================
 * 9. Persistent scan-line AR coding loop (csrc/scanline.hip): ONE launch walks all H*W coding steps of
 *    TopoGroupPGMPriorCoder._encode_with_pgm / _pgm_generate (pgm_coder.py:912-981) for the "scanline" topo groups
 *    (one position per group, raster order) with one channel group: masked k x k context convolution at the coded
 *    position (masked_conv.py:102-228: the causal raster neighbours), the dense 1x1 merger layers on cat(ctx, prior)
 *    (masked_conv.py:262-300 / pgm_coder.py:1606-1638), Gaussian index + quantise (pgm_coder.py:735-821,927-941).
 *    The layers' weights stay resident in the LDS of `workgroups` compute units for the whole launch.
 *    An encode launch may instead walk the rows of an image in parallel (the wavefront schedule, see
 *    basic_scanline_wavefront_max): W + (k / 2 + 2) * (H - 1) dependent steps, the same integers.
 * ==================================================================================== */
typedef struct basic_scanline_plan basic_scanline_plan;
/* ctx_weight [ctx_out][channels][k][k] (PyTorch layout; only the causal taps are used), ctx_bias [ctx_out] or NULL.
 * Dense layer i (i < n_dense): weight [dense_out[i]][in_i], in_0 = ctx_out + prior_channels (input = cat(ctx, prior)),
 * in_i = dense_out[i-1]; bias or NULL.  act_after[0] belongs to the context layer, act_after[1 + i] to dense layer i
 * (1 = LeakyReLU(0.01)).  The last layer must have 2 * channels rows: (mean, scale) pairs, channel 2c = mean.
 * dense_in_groups[i] (NULL = all 1): the input channel groups of the masked convolution dense layer i stands for
 * (masked_conv.py:170-172; cat(ctx, prior) of the first merger layer = 2): the sums are taken in that operator's canonical
 * block order (csrc/mconv.hip), so the integers coded here equal the per-step path's at any batch size. */
int basic_scanline_plan_create(const float *ctx_weight, const float *ctx_bias, int channels, int ctx_out, int ksize,
                               int prior_channels, int n_dense, const float *const *dense_weight,
                               const float *const *dense_bias, const int *dense_out, const int *act_after,
                               const int *dense_in_groups, basic_scanline_plan **out);
int basic_scanline_plan_info(const basic_scanline_plan *p, int *workgroups, int *lds_weight_bytes);
/* d_y [B][C][H][W], d_prior [B][prior_channels][H][W] (NULL when prior_channels == 0), d_table float32 [table_len]:
 * writes d_symbols / d_indexes int32 [B][H*W*C] in coding order (element p * C + c) and d_ybuf [B][C][H][W]
 * (= round(y - mu) + mu).  Enqueued on hip_stream; basic_scanline_status() afterwards tells whether every in-kernel
 * barrier completed (a launch whose grid was not fully resident gives up after a bounded spin instead of hanging). */
int basic_scanline_encode_dev(basic_scanline_plan *p, const float *d_y, const float *d_prior, int batch, int h, int w,
                              const float *d_table, int table_len, int32_t *d_symbols, int32_t *d_indexes, float *d_ybuf,
                              void *hip_stream);
/* Decoder: `tables` = the rANS table set of the coder; stream b = d_words[d_word_off[b] .. d_word_off[b+1]).  The
 * launch adds ceil(B / 4) decoder workgroups (one wavefront per image stream, the table set's search image in LDS) to the
 * compute workgroups; a coding step is: parameters (as in the encoder) -> table rows -> rANS decode of the C symbols of
 * that position -> y_hat = symbol + mean.  Writes d_symbols / d_indexes (coding order) and d_ybuf [B][C][H][W]. */
int basic_scanline_decode_dev(basic_scanline_plan *p, const basic_rans_tables *tables, const uint32_t *d_words,
                              const int64_t *d_word_off, const float *d_prior, int batch, int h, int w, const float *d_table,
                              int table_len, int32_t *d_symbols, int32_t *d_indexes, float *d_ybuf, void *hip_stream);
/* The decoder for LANE STREAMS (stream_lanes = `lanes`; not a format the reference reads): the channels are cut
 * into `lanes` runs of L = C / lanes (C % lanes == 0, L % 16 == 0), stream s = b * lanes + k = d_words[d_word_off[s] ..
 * d_word_off[s + 1]) carries image b's symbols of channels [k L, (k + 1) L) in coding order, and the launch adds
 * ceil(B * lanes / 4) decoder workgroups: one wavefront per lane stream, `lanes` of them decoding a position side by side.
 * Everything written is what basic_scanline_decode_dev writes; lanes == 1 IS basic_scanline_decode_dev. */
int basic_scanline_decode_lanes_dev(basic_scanline_plan *p, const basic_rans_tables *tables, const uint32_t *d_words,
                                    const int64_t *d_word_off, const float *d_prior, int batch, int lanes, int h, int w,
                                    const float *d_table, int table_len, int32_t *d_symbols, int32_t *d_indexes, float *d_ybuf,
                                    void *hip_stream);
/* basic_scanline_decode_lanes_dev for ROW STREAMS (stream_rows; not a format the reference reads): batch * h * lanes
 * streams, stream s = (b * h + r) * lanes + k = d_words[d_word_off[s] .. d_word_off[s + 1]) carries the symbols of row r of image
 * b, channels [k L, (k + 1) L), in coding order (lanes == 1: the whole row).  Where batch * h <= 64 columns and the compute
 * workgroups plus ceil(batch * h * lanes / 4) decoder workgroups are resident, the call may run as the WAVEFRONT decode launch
 * (w + (ksize / 2 + 2) * (h - 1) steps, one decoder wavefront per stream; BASIC_SCAN_KERNEL=wavefront forces it, "does not fit"
 * otherwise); else the raster kernels read the same streams, a decoder wavefront changing stream at every row start.
 * Under BASIC_SCAN_SCHEDULE_BAND (basic_scanline_set_decode_schedule) or BASIC_SCAN_KERNEL=band the call runs as the BAND decode
 * launch (basic_scanline_band_decode_max): the same steps for any batch and height, in as many launches as the batch needs.
 * Everything written is what basic_scanline_decode_dev writes. */
int basic_scanline_decode_rows_dev(basic_scanline_plan *p, const basic_rans_tables *tables, const uint32_t *d_words,
                                   const int64_t *d_word_off, const float *d_prior, int batch, int lanes, int h, int w,
                                   const float *d_table, int table_len, int32_t *d_symbols, int32_t *d_indexes, float *d_ybuf,
                                   void *hip_stream);
/* *ok = 1 when basic_scanline_decode_dev can serve `batch` streams of `tables` on the current device (fast search image that
 * fits the LDS; compute + decoder workgroups <= compute units); otherwise the caller decodes with the per-step path, which
 * codes the same integers. */
int basic_scanline_can_decode(const basic_scanline_plan *p, const basic_rans_tables *tables, int batch, int *ok);
/* Batches of 3 .. 64 images take the BATCHED persistent kernel when the layers have its shape (whole 32-row tiles and 64-channel
 * canonical blocks, <= 3 dense layers of <= 768 inputs, a context window of <= 36 blocks): the batch is the N dimension of
 * v_mfma_f32_32x32x2_f32 tiles, a workgroup keeps one row tile of a layer as A fragments in registers, 32 images per set of
 * workgroups.  *max_batch = the largest batch it serves for a latent `w` columns wide on the current device (0 = never);
 * decode != 0 counts the decoder workgroups too.  Which kernel serves a call never changes the coded integers. */
int basic_scanline_batched_max(const basic_scanline_plan *p, int w, int decode, int *max_batch);
/* ENCODE calls have a second schedule of the batched kernel, the WAVEFRONT: the causal k x k window orders a position only
 * after its left neighbour and the rows above, so row r may run s = k / 2 + 2 columns behind row r - 1.  A column of the MFMA
 * tiles is then one row of one image (B * H <= 64), step t codes column position t - s * r of every row r, and a launch walks
 * W + s * (H - 1) dependent steps instead of H * W (172 instead of 1,536 for a 32 x 48 latent).  The decoder cannot: it reads one
 * serial rANS stream.  The schedule never changes the coded integers or d_ybuf.
 * *max_batch = the largest batch the wavefront serves for an h x w latent on the current device; 0 = never (layers not of the
 * batched kernel's shape, h > 64, or a grid that is not resident).  Any width fits. */
int basic_scanline_wavefront_max(const basic_scanline_plan *p, int h, int w, int *max_batch);
/* A third encode schedule, the BAND, lifts the wavefront's B * H <= 64.  Row r of the wavefront is in flight only during steps
 * [s r, s r + w), so an image needs about w / s columns of the MFMA tiles, not h: it owns A = w / s + 1 column SLOTS of one
 * 32-column tile, slot j codes rows j, j + A, j + 2 A, ... back to back, and 32 / A images share a tile.  The steps stay
 * w + s * (h - 1) whatever the batch and the height; a launch runs up to 8 independent tiles, and a batch larger than one launch
 * holds is coded by successive launches over whole images inside the one basic_scanline_encode_dev call.  Same integers, same
 * d_ybuf; encode only.
 * *images_per_launch = the images one launch codes of an h x w latent on the current device; 0 = never (layers not of the
 * batched kernel's shape, A > 32 -- a latent wider than 31 * s columns --, or one image alone exceeds the scratch limit or the
 * kernel's 32-bit offsets).  Any batch fits when it is >= 1. */
int basic_scanline_band_max(const basic_scanline_plan *p, int h, int w, int *images_per_launch);
/* The BAND DECODE launch serves decode calls over ROW STREAMS (basic_scanline_decode_rows_dev) the same way: the band's compute
 * workgroups, plus one decoder wavefront per (image, slot, lane stream) -- slot j's wavefront decodes rows j, j + A, ... of its
 * image one after the other, changing stream in the slot's idle steps --, four to a workgroup, resident beside them.  An image
 * brings min(A, h) * lanes decoder wavefronts whatever its height, so the launch takes what the wavefront decode launch cannot:
 * more than 64 rows in all.  Opt-in: BASIC_SCAN_SCHEDULE_BAND as the plan's decode schedule, or BASIC_SCAN_KERNEL=band.
 * *images_per_launch = the largest n <= basic_scanline_band_max with
 *     tiles(n) * workgroups per tile + ceil(n * min(A, h) * lanes / 4) <= compute units;
 * 0 = never (also: `tables` has no fast search image that fits the LDS).  A larger batch takes several launches inside the call,
 * each with the decoder workgroups of its own images. */
int basic_scanline_band_decode_max(const basic_scanline_plan *p, const basic_rans_tables *tables, int h, int w, int lanes,
                                   int *images_per_launch);
/* *kernel = which kernel the plan's last launch (encode or decode) ran. */
#define BASIC_SCAN_KERNEL_NONE (-1) /* no launch yet */
#define BASIC_SCAN_KERNEL_GENERIC 0
#define BASIC_SCAN_KERNEL_PIPELINED 1
#define BASIC_SCAN_KERNEL_BATCHED 2
#define BASIC_SCAN_KERNEL_WAVEFRONT 3
#define BASIC_SCAN_KERNEL_BAND 4
int basic_scanline_last_kernel(const basic_scanline_plan *p, int *kernel);
/* How the plan's encode calls are scheduled from now on.  AUTO (the default): the wavefront where it fits and measured
 * faster; where it does not fit, the band where it measured faster and holds no more compute-unit time than the raster launch
 * (DESIGN.md section 3); else raster.  RASTER: the choice described at
 * basic_scanline_batched_max, never the wavefront or the band.  WAVEFRONT / BAND: always; a call that does not fit it fails
 * with BASIC_ERR_INVALID ("does not fit").  The environment variable
 * BASIC_SCAN_KERNEL = generic | pipelined | batched | wavefront | band, when set, wins over the plan's schedule; decode calls
 * ignore this schedule, and "wavefront" and "band" unless they bring row streams (basic_scanline_set_decode_schedule). */
#define BASIC_SCAN_SCHEDULE_AUTO 0
#define BASIC_SCAN_SCHEDULE_RASTER 1
#define BASIC_SCAN_SCHEDULE_WAVEFRONT 2
#define BASIC_SCAN_SCHEDULE_BAND 3
int basic_scanline_set_encode_schedule(basic_scanline_plan *p, int schedule);
/* How the plan's ROW-STREAM decode calls (basic_scanline_decode_rows_dev) are scheduled from now on, in the same values.  AUTO (the
 * default): the raster kernels -- no step cost of the wavefront or band decode launch has been turned into a rule yet.  RASTER:
 * never the wavefront or the band, whatever a later rule says.  WAVEFRONT / BAND: always that launch; a call that does not fit it
 * fails with BASIC_ERR_INVALID ("does not fit") before anything is launched.  BASIC_SCAN_KERNEL, when set, wins.
 * basic_scanline_decode_dev and basic_scanline_decode_lanes_dev cannot carry row streams and never look at this schedule (nor at
 * BASIC_SCAN_KERNEL=wavefront / band); basic_scanline_choose_rows with rows != 0 answers for it. */
int basic_scanline_set_decode_schedule(basic_scanline_plan *p, int schedule);
/* What a call would run, without launching anything: tables == NULL asks about basic_scanline_encode_dev, otherwise about
 * basic_scanline_decode_dev with that table set, for `batch` images of an h x w latent (0 = not known: only the kernels that
 * need no such knowledge are considered) and a scale table of table_len entries.  One planner in csrc/scanline.hip answers this
 * and plans the launches of both *_dev calls, so the answer is what they do.  `schedule` (BASIC_SCAN_SCHEDULE_*) stands for the
 * plan's encode schedule, BASIC_SCAN_KERNEL still wins over it, and lane_max_batch (>= 0) is the coder's gate: a larger batch is
 * not given to the kernels that keep one output per lane (generic, pipelined).
 * *kernel = BASIC_SCAN_KERNEL_*; BASIC_SCAN_KERNEL_NONE = leave the call to the per-step path (no persistent kernel serves the
 * batch, the grid would not be resident, or the table set has no fast search image).  *launches (may be NULL) = the launches of
 * the call: 1, or what the band needs for the batch.  A forced kernel or schedule that the call does not fit fails as the
 * launch would: BASIC_ERR_INVALID ("does not fit"). */
int basic_scanline_choose(const basic_scanline_plan *p, const basic_rans_tables *tables, int batch, int h, int w, int table_len,
                          int schedule, int lane_max_batch, int *kernel, int *launches);
/* basic_scanline_choose for a decode call over lane streams (basic_scanline_decode_lanes_dev): the decoder workgroups counted
 * are those of batch * lanes streams, so a call whose decoder wavefronts no longer fit beside the compute workgroups is left to
 * the per-step path.  Encode calls do not depend on `lanes`; lanes == 1 is basic_scanline_choose. */
int basic_scanline_choose_lanes(const basic_scanline_plan *p, const basic_rans_tables *tables, int batch, int lanes, int h, int w,
                                int table_len, int schedule, int lane_max_batch, int *kernel, int *launches);
/* basic_scanline_choose_lanes with `rows` != 0 for a decode call over row streams (basic_scanline_decode_rows_dev): the wavefront
 * decode launch is considered (its decoder workgroups: batch * h * lanes streams), the raster kernels count batch * lanes, and the
 * plan's decode schedule (basic_scanline_set_decode_schedule) holds as it does for the call.  Encode calls do not depend on `rows`;
 * rows == 0 is basic_scanline_choose_lanes. */
int basic_scanline_choose_rows(const basic_scanline_plan *p, const basic_rans_tables *tables, int batch, int lanes, int rows, int h, int w,
                               int table_len, int schedule, int lane_max_batch, int *kernel, int *launches);
int basic_scanline_status(basic_scanline_plan *p, void *hip_stream, int *poisoned);
void basic_scanline_plan_destroy(basic_scanline_plan *p);

/* ======================================================================================
 * 10. Table ANS (csrc/tans.hip) -- the drop-in for the reference's TansEncoder / TansDecoder
 *       class surface            csrc/ans/tans.hpp:78-157 (PYBIND11_TANS_CLASSES :146-157)
 *       TansBase::init_params    csrc/ans/tans.cpp:368-383, init_tables :385-525
 *       encode_with_indexes      csrc/ans/tans.cpp:527-680      flush :682-713
 *       decode_with_indexes      csrc/ans/tans.cpp:715-815
 *     Tables (count normalisation, state / symbol-transform / decode tables, tans.cpp:27-318) are built on the host
 *     and uploaded once; row `rows` of the images is the uniform bypass alphabet when bypass coding is on.
 *     freqs int32 [rows][freq_stride]; nsym / offsets int32 [rows]; table_log in [5, 12].
 * ==================================================================================== */
typedef struct basic_tans_tables basic_tans_tables;
int basic_tans_tables_create(const int32_t *freqs, int rows, int freq_stride, const int32_t *nsym, const int32_t *offsets,
                             int table_log, int max_symbol_value, int bypass_coding, int bypass_precision,
                             basic_tans_tables **out);
/* ANSBase::init_ar_params (csrc/ans/ans_interface.cpp:75-137), as basic_rans_tables_set_ar. */
int basic_tans_tables_set_ar(basic_tans_tables *t, const int32_t *ar_tab, int k, int rows, int order, int s1);
/* One row of the device images back on the host: next_state u16 [2^L], delta_bits / delta_state [nsym],
 * dec_packed u32 [2^L] = base | bits << 12 | symbol << 16 (any pointer may be NULL). */
int basic_tans_tables_get_row(const basic_tans_tables *t, int row, uint16_t *next_state, uint32_t *delta_bits,
                              int32_t *delta_state, uint32_t *dec_packed);
void basic_tans_tables_destroy(basic_tans_tables *t);
/* Host-buffer coder (arrays staged to HBM, coded by the HIP kernel, result copied back).  capacity_syms: the symbol
 * count the reference sizes its output with (-1 = n; flush(): the cached count incl. bypass digits): capacity
 * capacity_syms * table_log / 8 <= 8 bytes is its "Destination buffer is too small" error, a stream of capacity - 8
 * whole bytes or more comes back EMPTY there (bitstream.h:192,245) and here (*out_len = 0). */
int basic_tans_encode_host(const basic_tans_tables *t, const int32_t *symbols, const int32_t *indexes, int64_t n,
                           const int32_t *ar_indexes, const int32_t *ar_off0, const int32_t *ar_off1,
                           int64_t capacity_syms, uint8_t *out, int64_t out_capacity, int64_t *out_len, int64_t *coded_syms);
int basic_tans_decode_host(const basic_tans_tables *t, const uint8_t *stream, int64_t stream_len, const int32_t *indexes,
                           int64_t n, const int32_t *ar_indexes, const int32_t *ar_off0, const int32_t *ar_off1,
                           int32_t *out_symbols);
/* Batched device-pointer coder, one wavefront per stream (no AR remap).  Encoder: stream i goes LEFT-aligned into
 * d_out_words[i * slot_words ..] (slot_words >= basic_tans_encode_bound_words(t, longest stream));
 * d_out_info[2i] = its length in BITS incl. final state and end mark (-1 = slot overflow), d_out_info[2i+1] = symbols
 * coded incl. bypass digits; bytes = ceil(bits / 8).  Decoder: stream i = d_bytes[d_byte_off[i] .. d_byte_off[i+1]);
 * d_status[i] = 1 for an empty stream / missing end mark. */
int64_t basic_tans_encode_bound_words(const basic_tans_tables *t, int64_t n);
int basic_tans_encode_batch_dev(const basic_tans_tables *t, const int32_t *d_symbols, const int32_t *d_indexes,
                                const int64_t *d_seg, int nstreams, uint32_t *d_out_words, int64_t slot_words,
                                int64_t *d_out_info, void *hip_stream);
int basic_tans_decode_batch_dev(const basic_tans_tables *t, const uint8_t *d_bytes, const int64_t *d_byte_off,
                                const int32_t *d_indexes, const int64_t *d_seg, int nstreams, int32_t *d_out_symbols,
                                int32_t *d_status, void *hip_stream);
/* Which kernel the calling thread's last tANS launch was (host or device entry point): LDS = the state-dependent image is
 * copied to the LDS, GLOBAL = read from global memory (image over 144 KiB; host entry points: streams under 2048 symbols). */
#define BASIC_TANS_KERNEL_NONE (-1) /* no launch by this thread yet */
#define BASIC_TANS_KERNEL_ENC_LDS 0
#define BASIC_TANS_KERNEL_ENC_GLOBAL 1
#define BASIC_TANS_KERNEL_DEC_LDS 2
#define BASIC_TANS_KERNEL_DEC_GLOBAL 3
int basic_tans_last_launch(int *kernel);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_HIP_H */
