// Numerics of the split-bf16 convolution path (conv.hip, conv_split_bf16_kernel).
// 1. What does v_mfma_f32_32x32x16_bf16 compute?  D = C + sum of 16 exact bf16 x bf16 products, rounded how?
//    Candidates checked on random operands (products and C within a 2^12 range, so an fp64 sum is exact):
//      N  the exact sum rounded once to nearest-even      Z  the exact sum truncated once (towards zero)
//      S  C + p0 + p1 + ... + p15, each add rounded to nearest (k ascending, lane group 0 first)
// 2. Error of a 32 x 32 x K GEMM against fp64, as a fraction of sum_k |a b| per output (max and RMS over outputs), for
//      f32    the v_mfma_f32_32x32x2_f32 chain of the fp32 kernel
//      split6 three-piece split, the six products with i + j <= 2 smallest first into ONE accumulator (what conv.hip does)
//      split2 the same, with a0b0 in an accumulator of its own, added at the end
//    at the K of the targeted layers: 3200 (25 taps x 128), 1920 (15 x 128 and 10 x 192).
// Build: hipcc -O3 --offload-arch=gfx950 mfma_bf16_split.hip -o mfma_bf16_split ; run: ./mfma_bf16_split
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

// lane l: A row / B column l & 31, K values 8 (l >> 5) + j (j = 0..7) of each 16-deep step; C/D register r of lane l:
// row 8 (r >> 2) + 4 (l >> 5) + (r & 3), column l & 31
__device__ inline int drow(int r, int lane) { return 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3); }

__device__ inline void split3(float v, unsigned &h0, unsigned &h1, unsigned &h2)
{
    const unsigned a = __float_as_uint(v), a0 = a & 0xFFFF0000u;
    const unsigned r = __float_as_uint(v - __uint_as_float(a0)), r1 = r & 0xFFFF0000u;
    const unsigned s = __float_as_uint(__uint_as_float(r) - __uint_as_float(r1));
    h0 = a >> 16; h1 = r >> 16; h2 = s >> 16;
}

// A [32][K] row-major, B [K][32] row-major (fp32); mode 0: fp32 chain, 1: split6, 2: split2, 3: one bf16 MFMA on
// already-bf16 operands (part 1; K = 16)
__global__ void gemm(const float *A, const float *B, const float *C, float *D, int K, int mode)
{
    const int lane = threadIdx.x, col = lane & 31, kh = lane >> 5;
    f32x16 acc, acc0;
    for (int r = 0; r < 16; ++r) { acc[r] = C[drow(r, lane) * 32 + col]; acc0[r] = 0.f; }
    if (mode == 0) {
        for (int k = 0; k < K; k += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[col * K + k + kh], B[(k + kh) * 32 + col], acc, 0, 0, 0);
    } else {
        for (int k = 0; k < K; k += 16) {
            u32x4 ap[3], bp[3];
            for (int i = 0; i < 4; ++i) {
                unsigned a[2][3], b[2][3];
                for (int e = 0; e < 2; ++e) {
                    const int kk = k + 8 * kh + 2 * i + e;
                    split3(A[col * K + kk], a[e][0], a[e][1], a[e][2]);
                    split3(B[kk * 32 + col], b[e][0], b[e][1], b[e][2]);
                }
                for (int p = 0; p < 3; ++p) {
                    ap[p][i] = a[0][p] | (a[1][p] << 16);
                    bp[p][i] = b[0][p] | (b[1][p] << 16);
                }
            }
            auto mf = [](const u32x4 &x, const u32x4 &y, f32x16 c) {
                return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x), __builtin_bit_cast(bf16x8, y), c, 0, 0, 0);
            };
            if (mode == 3) { acc = mf(ap[0], bp[0], acc); continue; }
            acc = mf(ap[2], bp[0], acc);
            acc = mf(ap[1], bp[1], acc);
            acc = mf(ap[0], bp[2], acc);
            acc = mf(ap[1], bp[0], acc);
            acc = mf(ap[0], bp[1], acc);
            if (mode == 1) acc = mf(ap[0], bp[0], acc);
            else acc0 = mf(ap[0], bp[0], acc0);
        }
        if (mode == 2)
            for (int r = 0; r < 16; ++r) acc[r] += acc0[r];
    }
    for (int r = 0; r < 16; ++r) D[drow(r, lane) * 32 + col] = acc[r];
}

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint32_t next32() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return static_cast<uint32_t>(rs >> 11); }
static float bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static float bf16_rand(int lo_exp, int span)  // random bf16 value, exponent in [lo_exp, lo_exp + span)
{
    const uint32_t h = next32();
    return bits((h & 0x807F0000u) | (static_cast<uint32_t>(lo_exp + (h >> 8) % span) << 23));
}
static float f32_rand() { return static_cast<float>(static_cast<int32_t>(next32() << 1)) / 2147483648.0f; }

static int run(const std::vector<float> &A, const std::vector<float> &B, const std::vector<float> &C, std::vector<float> &D, int K, int mode)
{
    float *dA, *dB, *dC, *dD;
    CHECK(hipMalloc(&dA, A.size() * 4)); CHECK(hipMalloc(&dB, B.size() * 4)); CHECK(hipMalloc(&dC, 4096)); CHECK(hipMalloc(&dD, 4096));
    CHECK(hipMemcpy(dA, A.data(), A.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dB, B.data(), B.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dC, C.data(), 4096, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(gemm, dim3(1), dim3(64), 0, 0, dA, dB, dC, dD, K, mode);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(D.data(), dD, 4096, hipMemcpyDeviceToHost));
    CHECK(hipFree(dA)); CHECK(hipFree(dB)); CHECK(hipFree(dC)); CHECK(hipFree(dD));
    return 0;
}

int main()
{
    // ---- part 1: one bf16 MFMA
    long n_eq = 0, z_eq = 0, s_eq = 0, total = 0;
    for (int rep = 0; rep < 256; ++rep) {
        std::vector<float> A(32 * 16), B(16 * 32), C(1024), D(1024);
        for (auto &v : A) v = bf16_rand(124, 8);
        for (auto &v : B) v = bf16_rand(124, 8);
        for (int i = 0; i < 1024; ++i) C[i] = bits((next32() & 0x807FFFFFu) | (static_cast<uint32_t>(128 + next32() % 4) << 23));
        if (rep % 4 == 3)  // cancellation: C ~ -(sum of the products)
            for (int r = 0; r < 32; ++r)
                for (int c = 0; c < 32; ++c) {
                    double s = 0;
                    for (int k = 0; k < 16; ++k) s += static_cast<double>(A[r * 16 + k]) * B[k * 32 + c];
                    C[r * 32 + c] = -static_cast<float>(s) * (1.f + 0x1p-20f * static_cast<float>(next32() % 8));
                }
        if (run(A, B, C, D, 16, 3)) return 1;
        for (int r = 0; r < 32; ++r)
            for (int c = 0; c < 32; ++c) {
                double s = C[r * 32 + c];
                float seq = C[r * 32 + c];
                for (int k = 0; k < 16; ++k) {
                    const double p = static_cast<double>(A[r * 16 + k]) * B[k * 32 + c];
                    s += p;
                    seq = seq + static_cast<float>(p);  // p exact in fp32 (8 x 8 bits)
                }
                const float rn = static_cast<float>(s);
                float rz = rn;
                if (static_cast<double>(rn) != s && std::fabs(static_cast<double>(rn)) > std::fabs(s)) rz = std::nextafter(rn, 0.f);
                const float d = D[r * 32 + c];
                n_eq += d == rn; z_eq += d == rz; s_eq += d == seq; ++total;
            }
    }
    printf("v_mfma_f32_32x32x16_bf16, %ld outputs: equal to N (exact sum, one RNE) %ld | Z (exact sum, one truncation) %ld | "
           "S (sequential RNE adds) %ld\n", total, n_eq, z_eq, s_eq);

    // ---- part 2: GEMM error at the layers' K
    const int Ks[] = {3200, 1920};
    for (int K : Ks) {
        for (int dist = 0; dist < 2; ++dist) {  // 0: uniform (-1, 1) both; 1: activations |N|-like (>= 0), weights (-1, 1)
            std::vector<float> A(32 * static_cast<size_t>(K)), B(static_cast<size_t>(K) * 32), C(1024, 0.f), D(1024);
            for (auto &v : A) v = f32_rand() * 0.05f;
            for (auto &v : B) v = dist ? std::fabs(f32_rand() * f32_rand()) * 2.f : f32_rand();
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
            const char *names[] = {"f32", "split6", "split2"};
            printf("K %4d %s:", K, dist ? "act>=0 " : "uniform");
            for (int mode = 0; mode < 3; ++mode) {
                if (run(A, B, C, D, K, mode)) return 1;
                double emax = 0, e2 = 0;
                for (int i = 0; i < 1024; ++i) {
                    const double e = std::fabs(D[i] - ref[i]) / mag[i];
                    emax = e > emax ? e : emax;
                    e2 += e * e;
                }
                printf("  %s max %.3e rms %.3e", names[mode], emax, std::sqrt(e2 / 1024));
            }
            printf("   (errors / sum|ab|; 2^-24 = %.3e)\n", std::ldexp(1.0, -24));
        }
    }
    return 0;
}
