/*
 * satd_peak.hip -- what one SATD list pass of a 16x16 candidate costs a SIMD of a gfx950 CU, in the packed 16-bit body the analysis
 * kernel uses (pk_cols + satd4x4_half + group_sum) and as a product with the constant +-1 matrix on the matrix core.
 *
 * The matrix body: every pixel byte is XORed with 0x80 (u8 p -> i8 p - 128), one v_mfma_i32_16x16x32_i8 gets as its A operand
 * (16 rows of K = 32) the 16 source and the 16 reference pixels of sixteen 4x4 blocks, lane (m = lane & 15, g = lane >> 4) supplying
 * row g of block m (source dword low, reference dword high), and as its B operand [H16 ; -H16], H16 = H4 (x) H4.  The result is
 * D[m][n] = coefficient n of H16 (e - r) of block m (the two offsets cancel), lane (n, g) holding blocks 4g .. 4g+3.  With the
 * accumulator preset to a bias of 32768 every D lies in [28688, 36848], so v_sad_u16(D, bias, acc) is |coefficient| + acc in one
 * instruction.  Four instructions cover the 16 blocks of four 16x16 candidates (block m = 4 * candidate + block column, instruction
 * j = block row), so lane row g ends with candidate g's 4 coefficients-per-lane sums, and a 16-lane DPP sum finishes it.
 * A second matrix body starts from a zero accumulator and takes max(x, -x): no bias registers, more instructions.
 *
 * Timing as in valu_peak.hip: one workgroup per CU, 4 * W waves (W = 1, 2, 4 per SIMD), operands in registers, s_memtime around a
 * long stream of passes; cycles per pass per SIMD = (last end - first start) * 4 / passes of the workgroup, median over the CUs.
 * "mixed" runs four waves per SIMD, two of them the matrix body and two the packed one: whether the matrix pipe hides behind
 * other waves' VALU work.  Every wave reads the SIMD it runs on (HW_ID) and takes its body by its rank among the workgroup's waves
 * of that SIMD; the program reports in how many workgroups every SIMD really held the intended waves.  Before timing, the three bodies are compared on random bytes, all 0 against all 255 (both ways) and
 * the one-pixel checkerboards, and with a host computation of the same sums; a difference ends the program with status 1.
 *
 *   hipcc --offload-arch=gfx950 -O3 -o satd_peak tools/dbg/satd_peak.hip && timeout -k 10 120 ./satd_peak > profiles/satd_matrix_peak.json
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define PASSES_PER_TRIP 8
#define TRIPS 1024          /* 8192 passes per wave */

typedef short v2s __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
enum { BODY_PACKED, BODY_MFMA_BIAS, BODY_MFMA_ZERO, BODY_MIXED, N_BODIES };
static const char *const body_name[N_BODIES] = { "packed", "mfma_bias", "mfma_zero_max", "mixed_2_mfma_bias_2_packed" };

/* ---- the packed body: copies of pcamv_prims_gpu.h ---- */
__device__ __forceinline__ v2s as_v2s(uint32_t v) { return __builtin_bit_cast(v2s, v); }
__device__ __forceinline__ uint32_t as_u32(v2s v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ int dpp_qp1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false); }
__device__ __forceinline__ int dpp_qp2(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false); }
__device__ __forceinline__ int dpp_hmir(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false); }
__device__ __forceinline__ int dpp_mir(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false); }
__device__ __forceinline__ int group_sum16(int v) { v += dpp_qp1(v); v += dpp_qp2(v); v += dpp_hmir(v); v += dpp_mir(v); return v; }
__device__ __forceinline__ void pk_cols(const uint32_t r[4], uint32_t o[8])
{
#pragma unroll
    for (int x = 0; x < 4; x++) {
        const uint32_t sel = 0x0c040c00u + (uint32_t)x * 0x00010001u;
        o[x] = __builtin_amdgcn_perm(r[1], r[0], sel);
        o[4 + x] = __builtin_amdgcn_perm(r[3], r[2], sel);
    }
}
__device__ __forceinline__ int satd4x4_half(const uint32_t ec[8], const uint32_t r[4])
{
    uint32_t rc[8];
    pk_cols(r, rc);
    v2s t[8];
#pragma unroll
    for (int g = 0; g < 2; g++) {
        v2s d0 = as_v2s(ec[4 * g]) - as_v2s(rc[4 * g]), d1 = as_v2s(ec[4 * g + 1]) - as_v2s(rc[4 * g + 1]);
        v2s d2 = as_v2s(ec[4 * g + 2]) - as_v2s(rc[4 * g + 2]), d3 = as_v2s(ec[4 * g + 3]) - as_v2s(rc[4 * g + 3]);
        v2s s01 = d0 + d1, d01 = d0 - d1, s23 = d2 + d3, d23 = d2 - d3;
        t[4 * g] = s01 + s23; t[4 * g + 1] = d01 + d23; t[4 * g + 2] = s01 - s23; t[4 * g + 3] = d01 - d23;
    }
    v2s acc = {0, 0};
    const v2s z = {0, 0};
#pragma unroll
    for (int x = 0; x < 4; x++) {
        v2s S = t[x] + t[4 + x], D = t[x] - t[4 + x];
        v2s aS = __builtin_elementwise_max(S, z - S), aD = __builtin_elementwise_max(D, z - D);
        v2s U = as_v2s(__builtin_amdgcn_perm(as_u32(aD), as_u32(aS), 0x05040100u));
        v2s V = as_v2s(__builtin_amdgcn_perm(as_u32(aD), as_u32(aS), 0x07060302u));
        acc += __builtin_elementwise_max(U, V);
    }
    return (int)acc.x + (int)acc.y;
}
/* one pass: lane = candidate * 16 + block owns the block's four rows; every lane of a candidate gets its SATD */
__device__ __forceinline__ int pass_packed(const uint32_t ec[8], const uint32_t r[4]) { return group_sum16(satd4x4_half(ec, r)); }

/* ---- the matrix bodies ---- */
#define SATD_BIAS 32768
/* the lane's 8 bytes of B = [H16 ; -H16]: column n = lane & 15 (coefficient (a, b) = (n >> 2, n & 3)), k = 8g .. 8g+7 =
 * source pixels (row g, x = 0..3), then the reference pixels of that row with the opposite sign */
__device__ __forceinline__ long had_operand(int lane)
{
    const int n = lane & 15, g = lane >> 4, a = n >> 2, b = n & 3;
    uint32_t pat = b == 0 ? 0x01010101u : b == 1 ? 0xff01ff01u : b == 2 ? 0xffff0101u : 0x01ffff01u;
    if (__builtin_popcount(a & g) & 1) pat ^= 0xfefefefeu;        /* +1 <-> -1 in every byte */
    return (long)(((uint64_t)(pat ^ 0xfefefefeu) << 32) | pat);
}
/* e[j] (already XORed with 0x80808080), r[j]: row g of block (m, j).  Lane row g gets candidate g's SATD (x264's: half the sum) */
__device__ __forceinline__ int pass_mfma_bias(const uint32_t e[4], const uint32_t r[4], long hb)
{
    const v4i bias = {SATD_BIAS, SATD_BIAS, SATD_BIAS, SATD_BIAS};
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const long a = (long)(((uint64_t)(r[j] ^ 0x80808080u) << 32) | e[j]);
        const v4i d = __builtin_amdgcn_mfma_i32_16x16x32_i8(a, hb, bias, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; i++) s = __builtin_amdgcn_sad_u16((uint32_t)d[i], (uint32_t)SATD_BIAS, s);
    }
    return group_sum16((int)s) >> 1;
}
__device__ __forceinline__ int pass_mfma_zero(const uint32_t e[4], const uint32_t r[4], long hb)
{
    const v4i z = {0, 0, 0, 0};
    int s = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const long a = (long)(((uint64_t)(r[j] ^ 0x80808080u) << 32) | e[j]);
        const v4i d = __builtin_amdgcn_mfma_i32_16x16x32_i8(a, hb, z, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; i++) s += __builtin_elementwise_max(d[i], -d[i]);
    }
    return group_sum16(s) >> 1;
}

/* ---- equality check: 4 candidates, each a 16x16 source (as EV_SRC4 has them) against a 16x16 reference ---- */
__global__ void __launch_bounds__(64) k_check(const uint8_t *__restrict__ src, const uint8_t *__restrict__ ref, int *__restrict__ out)
{
    const int lane = threadIdx.x;
    uint32_t e[4], r[4], ec[8];
    {   /* packed: lane = candidate * 16 + block */
        const int c = lane >> 4, bx = lane & 3, by = (lane >> 2) & 3;
        for (int k = 0; k < 4; k++) {
            e[k] = *(const uint32_t *)(src + c * 256 + (4 * by + k) * 16 + 4 * bx);
            r[k] = *(const uint32_t *)(ref + c * 256 + (4 * by + k) * 16 + 4 * bx);
        }
        pk_cols(e, ec);
        const int v = pass_packed(ec, r);
        if ((lane & 15) == 0) out[c] = v;
    }
    {   /* matrix: lane (m, g) = row g of block (candidate m >> 2, column m & 3, block row j) */
        const int m = lane & 15, g = lane >> 4, c = m >> 2, bx = m & 3;
        for (int j = 0; j < 4; j++) {
            e[j] = *(const uint32_t *)(src + c * 256 + (4 * j + g) * 16 + 4 * bx) ^ 0x80808080u;
            r[j] = *(const uint32_t *)(ref + c * 256 + (4 * j + g) * 16 + 4 * bx);
        }
        const long hb = had_operand(lane);
        const int v = pass_mfma_bias(e, r, hb), w = pass_mfma_zero(e, r, hb);
        if ((lane & 15) == 0) { out[4 + g] = v; out[8 + g] = w; }
    }
}

/* ---- timing ---- */
template <int BODY> __global__ void __launch_bounds__(1024) k_satd_peak(unsigned long long *__restrict__ stamps, unsigned *__restrict__ sink, unsigned *__restrict__ place)
{
    extern __shared__ unsigned char pad[];          /* (only requested: one workgroup per CU) */
    __shared__ unsigned simd_rank[4];
    if (threadIdx.x < 4) simd_rank[threadIdx.x] = 0;
    __syncthreads();
    /* where the wave really runs: SIMD_ID = HW_ID[5:4] (hwreg 4); its rank among the workgroup's waves of that SIMD picks the body
     * of the mixed run, so that every SIMD gets as many matrix as packed waves however the dispatcher places them */
    const unsigned simd = __builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4);
    unsigned rank = 0;
    if ((threadIdx.x & 63) == 0) rank = atomicAdd(&simd_rank[simd], 1u);
    rank = (unsigned)__builtin_amdgcn_readfirstlane((int)rank);
    const int lane = threadIdx.x & 63;
    const unsigned wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    uint32_t e[4], r[4], ec[8];
    for (int k = 0; k < 4; k++) { e[k] = threadIdx.x * 2654435761u + k * 40503u; r[k] = threadIdx.x * 2246822519u + k * 69069u; }
    pk_cols(e, ec);
    const long hb = had_operand(lane);
    const bool packed = BODY == BODY_PACKED || (BODY == BODY_MIXED && (rank & 1));
    int acc = 0;
    __syncthreads();
    unsigned long long t0, t1;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0) :: "memory");
    if (packed) {
        for (int t = 0; t < TRIPS; t++)
#pragma unroll
            for (int p = 0; p < PASSES_PER_TRIP; p++) {
                asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]));      /* fresh reference rows as far as the compiler knows */
                acc += pass_packed(ec, r);
            }
    } else {
        for (int t = 0; t < TRIPS; t++)
#pragma unroll
            for (int p = 0; p < PASSES_PER_TRIP; p++) {
                asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]));
                acc += BODY == BODY_MFMA_ZERO ? pass_mfma_zero(e, r, hb) : pass_mfma_bias(e, r, hb);
            }
    }
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1) :: "memory");
    if (lane == 0) {                                /* ordinary vector stores, one lane per wave */
        stamps[2 * (blockIdx.x * waves + wave)] = t0;
        stamps[2 * (blockIdx.x * waves + wave) + 1] = t1;
        place[blockIdx.x * waves + wave] = simd | (packed ? 4u : 0u);
    }
    if (acc == 0x12345) sink[0] = (unsigned)acc;    /* keeps the stream alive */
}

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "satd_peak: %s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static int host_satd16(const uint8_t *s, const uint8_t *r)
{
    int sum = 0;
    for (int by = 0; by < 4; by++)
        for (int bx = 0; bx < 4; bx++) {
            int d[4][4], t[4][4];
            for (int y = 0; y < 4; y++)
                for (int x = 0; x < 4; x++) d[y][x] = (int)s[(4 * by + y) * 16 + 4 * bx + x] - (int)r[(4 * by + y) * 16 + 4 * bx + x];
            for (int y = 0; y < 4; y++) {
                const int s01 = d[y][0] + d[y][1], d01 = d[y][0] - d[y][1], s23 = d[y][2] + d[y][3], d23 = d[y][2] - d[y][3];
                t[y][0] = s01 + s23; t[y][1] = d01 + d23; t[y][2] = s01 - s23; t[y][3] = d01 - d23;
            }
            int b = 0;
            for (int x = 0; x < 4; x++) {
                const int s01 = t[0][x] + t[1][x], d01 = t[0][x] - t[1][x], s23 = t[2][x] + t[3][x], d23 = t[2][x] - t[3][x];
                b += abs(s01 + s23) + abs(d01 + d23) + abs(s01 - s23) + abs(d01 - d23);
            }
            sum += b >> 1;
        }
    return sum;
}

static int check(int *n_cases)
{
    /* per case 4 candidates: (source, reference) content by index */
    enum { C_RAND, C_0, C_255, C_CHK, C_CHKINV, C_VSTRIPE, C_HSTRIPE, C_127, C_128, N_C };
    static const int cases[][4][2] = {
        { {C_RAND, C_RAND}, {C_RAND, C_RAND}, {C_RAND, C_RAND}, {C_RAND, C_RAND} },
        { {C_0, C_255}, {C_255, C_0}, {C_CHK, C_CHKINV}, {C_CHKINV, C_CHK} },
        { {C_VSTRIPE, C_HSTRIPE}, {C_127, C_128}, {C_128, C_127}, {C_RAND, C_0} },
        { {C_RAND, C_255}, {C_CHK, C_RAND}, {C_HSTRIPE, C_VSTRIPE}, {C_0, C_0} },
    };
    const int nc = (int)(sizeof(cases) / sizeof(cases[0]));
    uint8_t *d_src, *d_ref; int *d_out;
    CHK(hipMalloc((void **)&d_src, 1024)); CHK(hipMalloc((void **)&d_ref, 1024)); CHK(hipMalloc((void **)&d_out, 12 * sizeof(int)));
    uint32_t seed = 12345u;
    int bad = 0;
    for (int k = 0; k < nc; k++) {
        uint8_t buf[2][1024];
        for (int c = 0; c < 4; c++)
            for (int w = 0; w < 2; w++)
                for (int i = 0; i < 256; i++) {
                    const int x = i & 15, y = i >> 4;
                    uint8_t v = 0;
                    switch (cases[k][c][w]) {
                    case C_RAND: seed = seed * 1664525u + 1013904223u; v = (uint8_t)(seed >> 24); break;
                    case C_0: v = 0; break;
                    case C_255: v = 255; break;
                    case C_CHK: v = ((x ^ y) & 1) ? 255 : 0; break;
                    case C_CHKINV: v = ((x ^ y) & 1) ? 0 : 255; break;
                    case C_VSTRIPE: v = (x & 1) ? 255 : 0; break;
                    case C_HSTRIPE: v = (y & 1) ? 255 : 0; break;
                    case C_127: v = 127; break;
                    case C_128: v = 128; break;
                    }
                    buf[w][c * 256 + i] = v;
                }
        int out[12];
        CHK(hipMemcpy(d_src, buf[0], 1024, hipMemcpyHostToDevice)); CHK(hipMemcpy(d_ref, buf[1], 1024, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_check, dim3(1), dim3(64), 0, 0, d_src, d_ref, d_out);
        CHK(hipGetLastError()); CHK(hipDeviceSynchronize());
        CHK(hipMemcpy(out, d_out, sizeof(out), hipMemcpyDeviceToHost));
        for (int c = 0; c < 4; c++) {
            const int h = host_satd16(buf[0] + c * 256, buf[1] + c * 256);
            if (out[c] != h || out[4 + c] != h || out[8 + c] != h) {
                fprintf(stderr, "satd_peak: case %d candidate %d: host %d packed %d mfma_bias %d mfma_zero_max %d\n", k, c, h, out[c], out[4 + c], out[8 + c]);
                bad++;
            }
        }
    }
    CHK(hipFree(d_src)); CHK(hipFree(d_ref)); CHK(hipFree(d_out));
    *n_cases = 4 * nc;
    return bad;
}

/* *even = workgroups whose every SIMD ran w waves (in the mixed run: w / 2 of either body) */
template <int BODY> static int measure(int cus, int w, unsigned long long *d_stamps, unsigned *d_sink, unsigned *d_place, double *out, int *even)
{
    const int waves = 4 * w;
    const size_t lds = 96 * 1024;                   /* of 160 KB: no second workgroup fits */
    CHK(hipFuncSetAttribute((const void *)k_satd_peak<BODY>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    std::vector<unsigned long long> h(2 * (size_t)cus * waves);
    for (int rep = 0; rep < 2; rep++) {             /* the first launch loads the code object and raises the clock */
        hipLaunchKernelGGL(k_satd_peak<BODY>, dim3(cus), dim3(64 * waves), lds, 0, d_stamps, d_sink, d_place);
        CHK(hipGetLastError());
        CHK(hipDeviceSynchronize());
    }
    CHK(hipMemcpy(h.data(), d_stamps, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
    std::vector<unsigned> pl((size_t)cus * waves);
    CHK(hipMemcpy(pl.data(), d_place, pl.size() * sizeof(pl[0]), hipMemcpyDeviceToHost));
    *even = 0;
    for (int b = 0; b < cus; b++) {
        int n[4] = {0, 0, 0, 0}, np[4] = {0, 0, 0, 0};
        for (int i = 0; i < waves; i++) { n[pl[b * waves + i] & 3]++; np[pl[b * waves + i] & 3] += (pl[b * waves + i] >> 2) & 1; }
        bool ok = true;
        for (int k = 0; k < 4; k++) ok = ok && n[k] == w && (BODY != BODY_MIXED || 2 * np[k] == w);
        *even += ok;
    }
    std::vector<double> per_wg(cus);
    for (int b = 0; b < cus; b++) {
        unsigned long long lo = ~0ull, hi = 0;
        for (int i = 0; i < waves; i++) { lo = std::min(lo, h[2 * (b * waves + i)]); hi = std::max(hi, h[2 * (b * waves + i) + 1]); }
        per_wg[b] = (double)(hi - lo) * 4.0 / ((double)waves * PASSES_PER_TRIP * TRIPS);
    }
    std::sort(per_wg.begin(), per_wg.end());
    *out = per_wg[cus / 2];
    return 0;
}

template <int BODY> static int sweep(int cus, unsigned long long *d_stamps, unsigned *d_sink, unsigned *d_place)
{
    double c[3];
    int ev[3];
    const int ws[3] = { 1, 2, 4 };
    for (int i = 0; i < 3; i++) if (measure<BODY>(cus, ws[i], d_stamps, d_sink, d_place, &c[i], &ev[i])) return 1;
    printf("  \"%s\": {\"1\": %.1f, \"2\": %.1f, \"4\": %.1f, \"workgroups_with_that_many_waves_on_every_simd\": [%d, %d, %d]},\n", body_name[BODY], c[0], c[1], c[2], ev[0], ev[1], ev[2]);
    return 0;
}

int main()
{
    hipDeviceProp_t p;
    CHK(hipGetDeviceProperties(&p, 0));
    const int cus = p.multiProcessorCount;
    int n_cases = 0;
    const int bad = check(&n_cases);
    if (bad) { fprintf(stderr, "satd_peak: %d of %d candidates differ between the bodies\n", bad, n_cases); return 1; }
    unsigned long long *d_stamps; unsigned *d_sink, *d_place;
    CHK(hipMalloc((void **)&d_stamps, sizeof(unsigned long long) * 2 * (size_t)cus * 16));
    CHK(hipMalloc((void **)&d_place, sizeof(unsigned) * (size_t)cus * 16));
    CHK(hipMalloc((void **)&d_sink, 64));
    printf("{\n \"what\": \"shader cycles (s_memtime) per SATD list pass (four 16x16 candidates, operands in registers) per SIMD, median over one workgroup per CU; keys = waves per SIMD\",\n");
    printf(" \"device\": \"%s\", \"arch\": \"%s\", \"compute_units\": %d, \"passes_per_wave\": %d,\n", p.name[0] ? p.name : "(no name reported by the runtime)", p.gcnArchName, cus, PASSES_PER_TRIP * TRIPS);
    printf(" \"bodies_equal_on\": \"%d candidates: random bytes, 0 / 255 both ways, one-pixel checkerboards both ways, stripes, 127 / 128; packed = mfma_bias = mfma_zero_max = host\",\n", n_cases);
    printf(" \"cycles_per_pass\": {\n");
    if (sweep<BODY_PACKED>(cus, d_stamps, d_sink, d_place) || sweep<BODY_MFMA_BIAS>(cus, d_stamps, d_sink, d_place) || sweep<BODY_MFMA_ZERO>(cus, d_stamps, d_sink, d_place)) return 1;
    double mixed;
    int even;
    if (measure<BODY_MIXED>(cus, 4, d_stamps, d_sink, d_place, &mixed, &even)) return 1;
    printf("  \"%s\": {\"4\": %.1f, \"workgroups_with_2_matrix_and_2_packed_waves_on_every_simd\": %d}\n }\n}\n", body_name[BODY_MIXED], mixed, even);
    CHK(hipFree(d_stamps)); CHK(hipFree(d_sink)); CHK(hipFree(d_place));
    return 0;
}
