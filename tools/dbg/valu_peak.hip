/*
 * valu_peak.hip -- how fast one SIMD of a gfx950 CU issues the integer wave64 instructions the analysis kernel is made of.
 *
 * One workgroup per CU (its LDS request keeps a second one off the CU), 4 * W waves in it (W = 1, 2, 4 per SIMD), every wave
 * a long unrolled stream of ONE instruction kind on eight independent registers.  Each wave stamps the cycle counter before
 * and after its stream; a workgroup's figure is  (last end - first start) * 4 SIMDs / wave-instructions issued by the
 * workgroup = cycles per wave-instruction per SIMD.  The median over the workgroups is printed as one JSON object.
 * DESIGN 4a quotes the result (profiles/r05_valu_peak.json) next to the 4 cycles `valu_issue_frac` assumes.
 *
 *   hipcc --offload-arch=gfx950 -O3 -o valu_peak tools/dbg/valu_peak.hip && ./valu_peak > valu_peak.json
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

#define UNROLL 64          /* instructions per loop trip: eight per register, round robin */
#define TRIPS 2048         /* 131072 instructions per wave: ~0.3 ms at 4 cycles each and 2.4 GHz */

enum { OP_ADD_U32, OP_SAD_U8, OP_PK_ADD_I16, OP_PERM_B32, OP_MOV_DPP, OP_READLANE, OP_MUL_U24, OP_LSHL_ADD, N_OPS };
static const char *const op_name[N_OPS] = { "v_add_u32", "v_sad_u8", "v_pk_add_i16", "v_perm_b32", "v_mov_b32_dpp", "v_readlane_b32",
                                            "v_mul_u32_u24", "v_lshl_add_u32" };

#define REP8(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
template <int OP> __device__ __forceinline__ void one(unsigned &r, unsigned k, unsigned &s)
{
    if (OP == OP_ADD_U32) asm volatile("v_add_u32 %0, %0, %1" : "+v"(r) : "v"(k));
    if (OP == OP_SAD_U8) asm volatile("v_sad_u8 %0, %0, %1, %0" : "+v"(r) : "v"(k));
    if (OP == OP_PK_ADD_I16) asm volatile("v_pk_add_i16 %0, %0, %1" : "+v"(r) : "v"(k));
    if (OP == OP_PERM_B32) asm volatile("v_perm_b32 %0, %0, %1, %1" : "+v"(r) : "v"(k));
    if (OP == OP_MOV_DPP) asm volatile("v_mov_b32_dpp %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "+v"(r));
    if (OP == OP_READLANE) asm volatile("v_readlane_b32 %0, %1, 5" : "=s"(s) : "v"(r));
    if (OP == OP_MUL_U24) asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(r) : "v"(k));
    if (OP == OP_LSHL_ADD) asm volatile("v_lshl_add_u32 %0, %0, 1, %1" : "+v"(r) : "v"(k));
}

template <int OP> __global__ void __launch_bounds__(1024) k_valu_peak(unsigned long long *__restrict__ stamps, unsigned *__restrict__ sink)
{
    extern __shared__ unsigned char pad[];          /* (only requested: one workgroup per CU) */
    unsigned r[8], s = 0, k = threadIdx.x | 1u;
    for (int i = 0; i < 8; i++) r[i] = threadIdx.x * 2654435761u + i;
    __syncthreads();
    unsigned long long t0, t1;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0) :: "memory");
    for (int t = 0; t < TRIPS; t++) {
#define STEP(i) one<OP>(r[i], k, s);
        REP8(STEP) REP8(STEP) REP8(STEP) REP8(STEP) REP8(STEP) REP8(STEP) REP8(STEP) REP8(STEP)
#undef STEP
    }
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1) :: "memory");
    unsigned acc = s;
    for (int i = 0; i < 8; i++) acc ^= r[i];
    const unsigned wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) {                  /* ordinary vector stores, one lane per wave */
        stamps[2 * (blockIdx.x * waves + wave)] = t0;
        stamps[2 * (blockIdx.x * waves + wave) + 1] = t1;
    }
    if (acc == 0x12345u) sink[0] = acc;             /* keeps the stream alive */
}

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "valu_peak: %s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <int OP> static int measure(int cus, int w, unsigned long long *d_stamps, unsigned *d_sink, double *out)
{
    const int waves = 4 * w;
    const size_t lds = 96 * 1024;                   /* of 160 KB: no second workgroup fits */
    CHK(hipFuncSetAttribute((const void *)k_valu_peak<OP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    std::vector<unsigned long long> h(2 * (size_t)cus * waves);
    for (int rep = 0; rep < 2; rep++) {             /* the first launch loads the code object and raises the clock */
        hipLaunchKernelGGL(k_valu_peak<OP>, dim3(cus), dim3(64 * waves), lds, 0, d_stamps, d_sink);
        CHK(hipGetLastError());
        CHK(hipDeviceSynchronize());
    }
    CHK(hipMemcpy(h.data(), d_stamps, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
    std::vector<double> per_wg(cus);
    for (int b = 0; b < cus; b++) {
        unsigned long long lo = ~0ull, hi = 0;
        for (int i = 0; i < waves; i++) { lo = std::min(lo, h[2 * (b * waves + i)]); hi = std::max(hi, h[2 * (b * waves + i) + 1]); }
        per_wg[b] = (double)(hi - lo) * 4.0 / ((double)waves * UNROLL * TRIPS);
    }
    std::sort(per_wg.begin(), per_wg.end());
    *out = per_wg[cus / 2];
    return 0;
}

template <int OP> static int sweep(int cus, unsigned long long *d_stamps, unsigned *d_sink, bool last)
{
    double c[3];
    const int ws[3] = { 1, 2, 4 };
    for (int i = 0; i < 3; i++) if (measure<OP>(cus, ws[i], d_stamps, d_sink, &c[i])) return 1;
    printf("  \"%s\": {\"1\": %.3f, \"2\": %.3f, \"4\": %.3f}%s\n", op_name[OP], c[0], c[1], c[2], last ? "" : ",");
    return 0;
}

int main()
{
    hipDeviceProp_t p;
    CHK(hipGetDeviceProperties(&p, 0));
    const int cus = p.multiProcessorCount;
    unsigned long long *d_stamps; unsigned *d_sink;
    CHK(hipMalloc((void **)&d_stamps, sizeof(unsigned long long) * 2 * (size_t)cus * 16));
    CHK(hipMalloc((void **)&d_sink, 64));
    printf("{\n \"what\": \"shader cycles (s_memtime) per wave64 instruction per SIMD, median over one workgroup per CU; keys = waves per SIMD\",\n");
    printf(" \"device\": \"%s\", \"arch\": \"%s\", \"compute_units\": %d, \"instructions_per_wave\": %d,\n \"cycles_per_wave_instruction\": {\n", p.name, p.gcnArchName, cus, UNROLL * TRIPS);
    if (sweep<OP_ADD_U32>(cus, d_stamps, d_sink, false) || sweep<OP_SAD_U8>(cus, d_stamps, d_sink, false) ||
        sweep<OP_PK_ADD_I16>(cus, d_stamps, d_sink, false) || sweep<OP_PERM_B32>(cus, d_stamps, d_sink, false) ||
        sweep<OP_MOV_DPP>(cus, d_stamps, d_sink, false) || sweep<OP_READLANE>(cus, d_stamps, d_sink, false) ||
        sweep<OP_MUL_U24>(cus, d_stamps, d_sink, false) || sweep<OP_LSHL_ADD>(cus, d_stamps, d_sink, true)) return 1;
    printf(" }\n}\n");
    CHK(hipFree(d_stamps)); CHK(hipFree(d_sink));
    return 0;
}
