// Numerics of the scaled two-piece fp16 split of the synthesis layers (conv.hip, conv_split_f16_kernel).
// 1. What does v_mfma_f32_32x32x16_f16 compute?  D = C + sum of 16 exact fp16 x fp16 products, rounded how?
//    Candidates checked on random operands (products and C within a 2^12 range, so an fp64 sum is exact):
//      N  the exact sum rounded once to nearest-even      Z  the exact sum truncated once (towards zero)
//      S  C + p0 + p1 + ... + p15, each add rounded to nearest (k ascending, lane group 0 first)
// 2. Are subnormal fp16 inputs used or flushed to zero?  A = 2^-20 (subnormal), B = 2^10, sixteen products: 16 x 2^-10 or 0.
// 3. Error of a 32 x 32 x K GEMM against fp64, as a fraction of sum_k |a b| per output (max and RMS over outputs), for
//      f32     the v_mfma_f32_32x32x2_f32 chain of the fp32 kernel
//      lo1st   scaled two-piece split, products a1b0, a0b1, a0b0 (smallest first) into one accumulator
//      hi1st   the same products as a0b0, a0b1, a1b0
//      lo1st2  smallest first, with a0b0 in an accumulator of its own, added at the end
//      noscale smallest first without the power-of-two scaling (what the low pieces lose to fp16's subnormal range)
//    Scaling: every A row (output channel) by the power of two that takes its max |a| into [2^13, 2^14), B (one image)
//    by the one that takes max |b| into [2^14, 2^15); undone exactly by ldexp at the end.
//    At the K of the targeted layers: 3200 (25 taps x 128), 1920 (15 x 128 and 10 x 192).
// Build: hipcc -O3 --offload-arch=gfx950 mfma_f16_split.hip -o mfma_f16_split ; run: ./mfma_f16_split
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

// lane l: A row / B column l & 31, K values 8 (l >> 5) + j (j = 0..7) of each 16-deep step; C/D register r of lane l:
// row 8 (r >> 2) + 4 (l >> 5) + (r & 3), column l & 31
__device__ inline int drow(int r, int lane) { return 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3); }

__device__ inline void split2(float v, _Float16 &h0, _Float16 &h1)
{
    h0 = static_cast<_Float16>(v);                           // round to nearest even
    h1 = static_cast<_Float16>(v - static_cast<float>(h0));  // the subtraction is exact
}

// A [32][K] row-major, B [K][32] row-major (fp32); ka[32]: power-of-two exponent per A row, kb: of B.
// mode 0: fp32 chain, 1: lo1st, 2: hi1st, 3: lo1st2, 4: one fp16 MFMA on operands that already are fp16 (K = 16)
__global__ void gemm(const float *A, const float *B, const float *C, float *D, int K, int mode, const int *ka, int kb)
{
    const int lane = threadIdx.x, col = lane & 31, kh = lane >> 5;
    f32x16 acc, acc0;
    for (int r = 0; r < 16; ++r) { acc[r] = C[drow(r, lane) * 32 + col]; acc0[r] = 0.f; }
    if (mode == 0) {
        for (int k = 0; k < K; k += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[col * K + k + kh], B[(k + kh) * 32 + col], acc, 0, 0, 0);
    } else {
        for (int k = 0; k < K; k += 16) {
            f16x8 a0, a1, b0, b1;
            for (int j = 0; j < 8; ++j) {
                const int kk = k + 8 * kh + j;
                _Float16 h0, h1;
                split2(ldexpf(A[col * K + kk], ka[col]), h0, h1);
                a0[j] = h0; a1[j] = h1;
                split2(ldexpf(B[kk * 32 + col], kb), h0, h1);
                b0[j] = h0; b1[j] = h1;
            }
            auto mf = [](const f16x8 &x, const f16x8 &y, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(x, y, c, 0, 0, 0); };
            if (mode == 4) { acc = mf(a0, b0, acc); continue; }
            if (mode == 2) {
                acc = mf(a0, b0, acc);
                acc = mf(a0, b1, acc);
                acc = mf(a1, b0, acc);
                continue;
            }
            acc = mf(a1, b0, acc);
            acc = mf(a0, b1, acc);
            if (mode == 1) acc = mf(a0, b0, acc);
            else acc0 = mf(a0, b0, acc0);
        }
        if (mode == 3)
            for (int r = 0; r < 16; ++r) acc[r] += acc0[r];
        if (mode != 4)
            for (int r = 0; r < 16; ++r) acc[r] = ldexpf(acc[r], -(ka[drow(r, lane)] + kb));
    }
    for (int r = 0; r < 16; ++r) D[drow(r, lane) * 32 + col] = acc[r];
}

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint32_t next32() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return static_cast<uint32_t>(rs >> 11); }
static float bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static float f16_rand(int lo_exp, int span)  // random fp16-representable value (11 significant bits), exponent in [lo_exp, lo_exp + span)
{
    const uint32_t h = next32();
    return bits((h & 0x807FE000u) | (static_cast<uint32_t>(lo_exp + (h >> 8) % span) << 23));
}
static float f32_rand() { return static_cast<float>(static_cast<int32_t>(next32() << 1)) / 2147483648.0f; }

static int run(const std::vector<float> &A, const std::vector<float> &B, const std::vector<float> &C, std::vector<float> &D, int K, int mode,
               const std::vector<int> &ka, int kb)
{
    float *dA, *dB, *dC, *dD;
    int *dk;
    CHECK(hipMalloc(&dA, A.size() * 4)); CHECK(hipMalloc(&dB, B.size() * 4)); CHECK(hipMalloc(&dC, 4096)); CHECK(hipMalloc(&dD, 4096));
    CHECK(hipMalloc(&dk, 128));
    CHECK(hipMemcpy(dA, A.data(), A.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dB, B.data(), B.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dC, C.data(), 4096, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dk, ka.data(), 128, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(gemm, dim3(1), dim3(64), 0, 0, dA, dB, dC, dD, K, mode, dk, kb);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(D.data(), dD, 4096, hipMemcpyDeviceToHost));
    CHECK(hipFree(dA)); CHECK(hipFree(dB)); CHECK(hipFree(dC)); CHECK(hipFree(dD)); CHECK(hipFree(dk));
    return 0;
}

// the power of two that takes m into [2^top, 2^(top + 1)); 0 for m = 0
static int scale_exp(float m, int top)
{
    if (!(m > 0.f) || !std::isfinite(m)) return 0;
    int e;
    std::frexp(m, &e);  // m in [2^(e - 1), 2^e)
    return top - (e - 1);
}

int main()
{
    const std::vector<int> k0(32, 0);
    // ---- part 1: one fp16 MFMA
    long n_eq = 0, z_eq = 0, s_eq = 0, total = 0;
    for (int rep = 0; rep < 256; ++rep) {
        std::vector<float> A(32 * 16), B(16 * 32), C(1024), D(1024);
        for (auto &v : A) v = f16_rand(124, 8);
        for (auto &v : B) v = f16_rand(124, 8);
        for (int i = 0; i < 1024; ++i) C[i] = bits((next32() & 0x807FFFFFu) | (static_cast<uint32_t>(128 + next32() % 4) << 23));
        if (rep % 4 == 3)  // cancellation: C ~ -(sum of the products)
            for (int r = 0; r < 32; ++r)
                for (int c = 0; c < 32; ++c) {
                    double s = 0;
                    for (int k = 0; k < 16; ++k) s += static_cast<double>(A[r * 16 + k]) * B[k * 32 + c];
                    C[r * 32 + c] = -static_cast<float>(s) * (1.f + 0x1p-20f * static_cast<float>(next32() % 8));
                }
        if (run(A, B, C, D, 16, 4, k0, 0)) return 1;
        for (int r = 0; r < 32; ++r)
            for (int c = 0; c < 32; ++c) {
                double s = C[r * 32 + c];
                float seq = C[r * 32 + c];
                for (int k = 0; k < 16; ++k) {
                    const double p = static_cast<double>(A[r * 16 + k]) * B[k * 32 + c];
                    s += p;
                    seq = seq + static_cast<float>(p);  // p exact in fp32 (11 x 11 bits)
                }
                const float rn = static_cast<float>(s);
                float rz = rn;
                if (static_cast<double>(rn) != s && std::fabs(static_cast<double>(rn)) > std::fabs(s)) rz = std::nextafter(rn, 0.f);
                const float d = D[r * 32 + c];
                n_eq += d == rn; z_eq += d == rz; s_eq += d == seq; ++total;
            }
    }
    printf("v_mfma_f32_32x32x16_f16, %ld outputs: equal to N (exact sum, one RNE) %ld | Z (exact sum, one truncation) %ld | "
           "S (sequential RNE adds) %ld\n", total, n_eq, z_eq, s_eq);

    // ---- part 2: subnormal fp16 inputs
    {
        std::vector<float> A(32 * 16, 0x1p-20f), B(16 * 32, 0x1p10f), C(1024, 0.f), D(1024);
        if (run(A, B, C, D, 16, 4, k0, 0)) return 1;
        printf("subnormal fp16 inputs: 16 x (2^-20 x 2^10) = %g (used: %g, flushed: 0)\n", D[0], 16 * 0x1p-10);
    }

    // ---- part 3: GEMM error at the layers' K
    const int Ks[] = {3200, 1920};
    int gate_ok = 1;
    for (int K : Ks) {
        for (int dist = 0; dist < 4; ++dist) {  // activations: 0 uniform (-1, 1); 1 |N|-like >= 0; 2, 3 the same x 2^-10
            std::vector<float> A(32 * static_cast<size_t>(K)), B(static_cast<size_t>(K) * 32), C(1024, 0.f), D(1024);
            for (auto &v : A) v = f32_rand() * 0.05f;
            for (auto &v : B) v = ((dist & 1) ? std::fabs(f32_rand() * f32_rand()) * 2.f : f32_rand()) * ((dist & 2) ? 0x1p-10f : 1.f);
            std::vector<int> ka(32);
            float bmax = 0.f;
            for (int r = 0; r < 32; ++r) {
                float m = 0.f;
                for (int k = 0; k < K; ++k) m = std::fmax(m, std::fabs(A[r * static_cast<size_t>(K) + k]));
                ka[r] = scale_exp(m, 13);
            }
            for (auto &v : B) bmax = std::fmax(bmax, std::fabs(v));
            const int kb = scale_exp(bmax, 14);
            std::vector<double> ref(1024), mag(1024);
            for (int r = 0; r < 32; ++r)
                for (int c = 0; c < 32; ++c) {
                    double s = 0, m = 0;
                    for (int k = 0; k < K; ++k) {
                        const double p = static_cast<double>(A[r * static_cast<size_t>(K) + k]) * B[static_cast<size_t>(k) * 32 + c];
                        s += p; m += std::fabs(p);
                    }
                    ref[r * 32 + c] = s; mag[r * 32 + c] = m;
                }
            const char *names[] = {"f32", "lo1st", "hi1st", "lo1st2", "noscale"};
            const char *dn[] = {"uniform      ", "act>=0       ", "uniform 2^-10", "act>=0  2^-10"};
            printf("K %4d %s:", K, dn[dist]);
            double rms_f32 = 0;
            for (int col = 0; col < 5; ++col) {
                const int mode = col == 4 ? 1 : col;
                if (run(A, B, C, D, K, mode, col == 4 ? k0 : ka, col == 4 ? 0 : kb)) return 1;
                double emax = 0, e2 = 0;
                for (int i = 0; i < 1024; ++i) {
                    const double e = std::fabs(D[i] - ref[i]) / mag[i];
                    emax = e > emax ? e : emax;
                    e2 += e * e;
                }
                const double rms = std::sqrt(e2 / 1024);
                if (col == 0) rms_f32 = rms;
                if (col == 1 && rms > 1.5 * rms_f32) gate_ok = 0;
                printf("  %s max %.3e rms %.3e", names[col], emax, rms);
                if (col) printf(" (%.2fx)", rms / rms_f32);
            }
            printf("\n");
        }
    }
    printf("(errors / sum|ab|; 2^-24 = %.3e)  gate, lo1st rms <= 1.5 x f32 rms in every row: %s\n", std::ldexp(1.0, -24), gate_ok ? "holds" : "FAILS");
    return 0;
}
