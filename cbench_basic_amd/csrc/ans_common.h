// What the two stream coders (rans.hip, tans.hip) share around their kernel loops: the AR remap of a symbol's table row, the
// bypass split of a value and its digit count, and the staging of a single-stream host call.
#pragma once
#include "common.h"

namespace basic {

// ---------------------------------------------------------------------------------------
// Device side
// ---------------------------------------------------------------------------------------
struct ArDev {
    const int32_t *tab;  // nullptr = no AR remap
    int k, order, rows, s1;
    const int32_t *ar_indexes, *off0, *off1;  // per stream-element arrays (global element ids)
    const int32_t *off2;                       // third back distance (custom ops only)
    int custom;                                // tab = float [k][7]: w0 w1 w2 bias scale min max (init_custom_ar_ops)
};

__device__ __forceinline__ int32_t clampi(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// AR remap of the table row (ans_interface.hpp:89-104); every index is clamped so that a
// malformed input can never read outside the tables.
__device__ __forceinline__ int32_t ar_row(const ArDev &ar, int32_t a, int32_t row, int32_t v0, int32_t v1)
{
    a = clampi(a, 0, ar.k - 1);
    row = clampi(row, 0, ar.rows - 1);
    v0 = clampi(v0, 0, ar.s1 - 1);
    if (ar.order == 1) return ar.tab[(static_cast<int64_t>(a) * ar.rows + row) * ar.s1 + v0];
    v1 = clampi(v1, 0, ar.s1 - 1);
    return ar.tab[((static_cast<int64_t>(a) * ar.rows + row) * ar.s1 + v0) * ar.s1 + v1];
}

// ar_limited_scaled_add_linear_op::op on (index, the RAW previous symbols), csrc/ans/ar_funcs.hpp:58-87 called from
// ar_update_index (ans_interface.hpp:60-84).  float arithmetic with every product and sum rounded on its own, as the
// reference's x86 build does (no fused multiply-add: the intrinsics keep hipcc from contracting).
__device__ __forceinline__ int32_t ar_custom_row(const ArDev &ar, int32_t a, int32_t row, int32_t v0, int32_t v1, int32_t v2)
{
    const float *op = reinterpret_cast<const float *>(ar.tab) + static_cast<int64_t>(clampi(a, 0, ar.k - 1)) * 7;
    const float base = static_cast<float>(row), scale = op[4];
    const float base_unscaled = floorf(__fdiv_rn(base, scale));
    float adder = __fadd_rn(0.f, __fmul_rn(static_cast<float>(v0), op[0]));
    if (ar.order > 1) adder = __fadd_rn(adder, __fmul_rn(static_cast<float>(v1), op[1]));
    if (ar.order > 2) adder = __fadd_rn(adder, __fmul_rn(static_cast<float>(v2), op[2]));
    adder = __fadd_rn(adder, op[3]);
    float lim = __fadd_rn(base_unscaled, adder);
    lim = lim < op[6] ? lim : op[6];
    lim = op[5] > lim ? op[5] : lim;
    const float step = __fmul_rn(__fsub_rn(roundf(lim), base_unscaled), scale);
    return static_cast<int32_t>(__fadd_rn(base, step));
}

// The row of element e of a stream (global element g) from its one to three predecessors, `off*[g]` elements back;
// load(k) = symbol k of the same stream (an encoder's input, a decoder's output so far), a distance that is not positive or
// reaches in front of the stream = no predecessor.  kCustomOps = false leaves the custom ops (and with them the third
// predecessor) out of the generated code: tANS table sets never carry them.
template <bool kCustomOps, class Load>
__device__ __forceinline__ int32_t ar_remap_row(const ArDev &ar, int32_t row, int64_t g, int64_t e, Load &&load)
{
    const int32_t a = ar.ar_indexes ? ar.ar_indexes[g] : 0;
    const int32_t one = kCustomOps && ar.custom ? 0 : 1;   // the table flavour indexes with symbol + 1 (0 = no predecessor)
    const int32_t d0 = ar.off0[g];
    const int32_t v0 = (d0 > 0 && d0 <= e) ? load(e - d0) + one : 0;
    int32_t v1 = 0, v2 = 0;
    if (ar.order >= 2) {
        const int32_t d1 = ar.off1[g];
        v1 = (d1 > 0 && d1 <= e) ? load(e - d1) + one : 0;
    }
    if (kCustomOps && ar.order >= 3) {
        const int32_t d2 = ar.off2[g];
        v2 = (d2 > 0 && d2 <= e) ? load(e - d2) + one : 0;
    }
    return kCustomOps && ar.custom ? ar_custom_row(ar, a, row, v0, v1, v2) : ar_row(ar, a, row, v0, v1);
}

// A value outside [0, max_value) is coded as the sentinel max_value followed by `raw`: odd for a negative value, even for a
// high one (rans64.cpp:312-339; the tANS encoder splits the same way).
__device__ __forceinline__ void bypass_split(int32_t &value, int32_t max_value, uint32_t &raw)
{
    int32_t v = value;   // on copies: stores through the references under a condition would reach the callers as branches
    uint32_t r = raw;
    if (v < 0) { r = static_cast<uint32_t>(-2 * v - 1); v = max_value; }
    else if (v >= max_value) { r = static_cast<uint32_t>(2 * (v - max_value)); v = max_value; }
    value = v;
    raw = r;
}

// digits of bprec bits that the escape code of `raw` holds
__device__ __forceinline__ int escape_digits(uint32_t r, uint32_t bprec)
{
    int nb = 0;
    while (nb * bprec < 32u && (r >> (nb * bprec)) != 0u) ++nb;
    return nb;
}

// ---------------------------------------------------------------------------------------
// Host side: staging of the host-buffer entry points (one stream per call, a hipMalloc per array)
// ---------------------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
    template <typename T> T *as() { return static_cast<T *>(p); }
};

template <typename T> hipError_t upload(DevBuf &b, const T *src, size_t n)
{
    const hipError_t e = b.alloc(n * sizeof(T));
    return e != hipSuccess || n == 0 ? e : hipMemcpy(b.p, src, n * sizeof(T), hipMemcpyHostToDevice);
}

// The AR part of a table set (basic_rans_tables, basic_tans_tables); tab == nullptr: none.
struct ArSource {
    const int32_t *tab;
    int k, order, rows, s1;
    bool custom;
};

struct ArBufs { DevBuf ai, o0, o1, o2; };

inline int stage_ar(const ArSource &src, int64_t n, const int32_t *ar_indexes, const int32_t *off0, const int32_t *off1,
                    const int32_t *off2, ArBufs &b, ArDev &ar)
{
    ar = ArDev{};
    if (!src.tab) return BASIC_OK;
    if (!off0 || (!src.custom && src.order == 2 && !off1)) {
        set_error("ar_offsets is required for ar coding!");
        return BASIC_ERR_INVALID;
    }
    ar.tab = src.tab; ar.k = src.k; ar.order = src.order; ar.rows = src.rows; ar.s1 = src.s1;
    if (src.custom) {   // the op's arity is the number of offset rows of this call (ans_interface.hpp:70-84)
        ar.custom = 1;
        ar.order = off2 ? 3 : off1 ? 2 : 1;
        if (off2 && !off1) { set_error("ar_offsets rows must be given in order"); return BASIC_ERR_INVALID; }
    }
    const size_t count = static_cast<size_t>(n);
    if (ar_indexes) { BASIC_HIP_TRY(upload(b.ai, ar_indexes, count)); ar.ar_indexes = b.ai.as<int32_t>(); }
    BASIC_HIP_TRY(upload(b.o0, off0, count));
    ar.off0 = b.o0.as<int32_t>();
    if (ar.order >= 2) { BASIC_HIP_TRY(upload(b.o1, off1, count)); ar.off1 = b.o1.as<int32_t>(); }
    if (ar.order >= 3) { BASIC_HIP_TRY(upload(b.o2, off2, count)); ar.off2 = b.o2.as<int32_t>(); }
    return BASIC_OK;
}

// Device buffers of a single-stream host call: the stream's n symbols (an encoder's input; symbols == nullptr: room for a
// decoder's result), their table rows, the segment {0, n}, and the AR arrays of stage_ar.
struct HostCall {
    DevBuf sym, idx, seg;
    ArBufs ar;
    size_t n = 0;
    int stage(const int32_t *symbols, const int32_t *indexes, int64_t count)
    {
        n = static_cast<size_t>(count);
        const int64_t s[2] = {0, count};
        BASIC_HIP_TRY(symbols ? upload(sym, symbols, n) : sym.alloc(n * sizeof(int32_t)));
        BASIC_HIP_TRY(upload(idx, indexes, n));
        BASIC_HIP_TRY(upload(seg, s, 2));
        return BASIC_OK;
    }
    int fetch(int32_t *out_symbols)   // the decoded symbols
    {
        if (n) BASIC_HIP_TRY(hipMemcpy(out_symbols, sym.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        return BASIC_OK;
    }
};

}  // namespace basic
