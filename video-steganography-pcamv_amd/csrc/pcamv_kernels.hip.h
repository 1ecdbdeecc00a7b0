/*
 * pcamv_kernels.hip.h -- the kernels of the analysis and of the second pass that the main unit, pcamv_gpu.hip, launches (gfx950;
 * plane production: pcamv_planes.hip.h, embedding and receiver: pcamv_embed.hip.h).  Only pcamv_gpu.hip includes this header.
 *
 *   k_search_diag / k_rca / k_encode     PCAMV_SCHED=diag: phase A for one anti-diagonal, one wavefront per macroblock; phase B,
 *                     one wavefront per (macroblock, carrier slot); phase C, one wavefront per macroblock
 *                     (the second pass and the loop filter of one anti-diagonal: pcamv_pass2_diag.hip)
 *   k_flow_init       queue and dependency counters of a persistent launch
 *   k_analyse_flow    the dataflow schedule of the analysis, common instance (the --me tesa and RD instances: pcamv_tesa.hip, pcamv_rd.hip)
 *   k_pass2_deblock_flow   second pass + loop filter through the same queue, a run of macroblocks per task
 *   k_block_costs / k_rd_probe   probes of the pixel metrics for parity tests through the C ABI
 */
#ifndef PCAMV_KERNELS_HIP_H
#define PCAMV_KERNELS_HIP_H
#include "pcamv_flow.hip.h"

/* ------------------------------------------------------------------ analysis phases */
template <int VARIANT>
__global__ void __launch_bounds__(64) k_search_diag(const FrameDev *__restrict__ Fs, int d)
{
    __shared__ MBLocal L;
    __shared__ Analysis A;
    const FrameDev F = Fs[blockIdx.y];
    int x, y;
    if (!diag_pos(F, d, &x, &y)) return;
    mbk_search<VARIANT>(F, &L, &A, x, y);
}
static __global__ void __launch_bounds__(64) k_rca(const FrameDev *__restrict__ Fs, int slots_per_mb)
{
    __shared__ MBLocal L;
    __shared__ Analysis A;
    const FrameDev F = Fs[blockIdx.y];
    if (!F.embed) return;
    int xy = blockIdx.x / slots_per_mb, k = blockIdx.x - xy * slots_per_mb;
    if (xy >= F.n_mb) return;
    mbk_rca(F, &L, &A, xy, k);
}
static __global__ void __launch_bounds__(64) k_encode(const FrameDev *__restrict__ Fs)
{
    __shared__ MBLocal L;
    __shared__ Analysis A;
    const FrameDev F = Fs[blockIdx.y];
    if ((int)blockIdx.x >= F.n_mb) return;
    mbk_encode(F, &L, &A, blockIdx.x);
}

/* ------------------------------------------------------------------ the persistent kernels (pcamv_flow.hip.h) */
static __global__ void __launch_bounds__(256) k_flow_init(FlowDev fl)
{
    unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= fl.total) return;
    int xy = (int)(i % (unsigned)fl.n_mb), x = xy % fl.mb_w, y = xy / fl.mb_w;
    fl.dep[i] = fl.raster ? (xy > 0) : (x > 0) + (y > 0);
    /* word i of the queue array is entry k of queue q; the first ngop(q) entries of each queue start out
     * published: macroblock 0 of the GOPs k * nq + q */
    int q = 0;
    while (q + 1 < fl.nq && i >= fl.qbase[q + 1]) q++;
    const unsigned k = i - fl.qbase[q], ngop_q = fl.qcount[q] / (unsigned)fl.n_mb;
    fl.queue[i] = k < ngop_q ? ((k * (unsigned)fl.nq + (unsigned)q) << 16) + 1u : 0u;
    if (i < 8) { fl.ctr[FLOW_HEAD(i)] = 0u; fl.ctr[FLOW_TAIL(i)] = fl.qcount[i] / (unsigned)fl.n_mb; }     /* heads 0, tails = GOPs of the queue; the error flag is the host's */
    if (fl.spec && i < (unsigned)fl.n_gop) fl.rdone[FLOW_RDONE_STRIDE * i] = 0u;
}
static __global__ void __launch_bounds__(64, PCAMV_FLOW_OCC) k_analyse_flow(const FrameDev *__restrict__ Fs, FlowDev fl)
{
    __shared__ MBLocal L;
    __shared__ Analysis A;
    flow_loop<0, 0>(Fs, fl, L, &A, nullptr);
}

/* pass 2 + loop filter through the same queue: the tasks are short (~5 us), which only works because the hand-off
 * costs no cache maintenance -- final motion and reconstructed pixels are stored write-through (NB_ST*) and the
 * filter reads its neighbourhood with agent-scope loads (NB_LD*).  (With an agent-scope release + acquire per
 * macroblock this was slower than one launch per anti-diagonal: 245 vs 176 ms per closed-loop step at G=256.) */
#ifndef PCAMV_PASS2_OCC
#define PCAMV_PASS2_OCC 4         /* waves per SIMD the second-pass kernel's registers are held to (its LDS -- the tile of a run of macroblocks -- allows four) */
#endif
static __global__ void __launch_bounds__(64, PCAMV_PASS2_OCC) k_pass2_deblock_flow(const FrameDev *__restrict__ Fs, FlowDev fl)
{
    /* only the head of the per-macroblock storage (PCAMV_PASS2_LDS: the fields the second pass touches come first in MBLocal): 4.3 instead
     * of 8.9 KB per wave */
    __shared__ __attribute__((aligned(16))) uint8_t Lraw[PCAMV_PASS2_LDS];
    __shared__ __attribute__((aligned(16))) P2Unit U;
    flow_loop<1, 0>(Fs, fl, *reinterpret_cast<MBLocal *>(Lraw), nullptr, &U);
}

/* block-cost probe: the pixel metrics of a1/a2/a5/a6 (SAD, SATD, qpel fetch, chroma MC) at arbitrary
 * positions, for checkasm-style parity tests through the C ABI.  req = {mb_x,mb_y,ip,xoff,yoff,mx,my,satd} */
static __global__ void __launch_bounds__(64) k_block_costs(const FrameDev *__restrict__ Fs, const int *__restrict__ req, int *__restrict__ out)
{
    __shared__ MBLocal L;
    const FrameDev F = Fs[0];
    const int *r = req + 8 * blockIdx.x;
    L.mb_x = r[0]; L.mb_y = r[1]; L.mb_xy = r[1] * F.mb_w + r[0];
    prim_load_fenc(F, &L);
    PCAMV_WAVE_SYNC();
    const int mflag = (r[7] & 1 ? EV_SATD : 0) | EV_NOMV;
    if (r[7] & 2) {     /* batch mode: 4 candidates around (mx,my) in one list; answer = 3 of them */
        if (LANE() == 0) {
            L.cxy[0] = CAND_PACK(r[5], r[6]); L.cxy[1] = CAND_PACK(r[5] + 1, r[6] - 1);
            L.cxy[2] = CAND_PACK(r[5] - 2, r[6] + 3); L.cxy[3] = CAND_PACK(r[5] + 3, r[6] + 2);
        }
        prim_eval_list(F, &L, L.fenc, r[2], r[3], r[4], 4, mflag, 0, 0);
        if (LANE() == 0) { out[3 * blockIdx.x] = L.ccost[1]; out[3 * blockIdx.x + 1] = L.ccost[2]; out[3 * blockIdx.x + 2] = L.ccost[3]; }
        return;
    }
    if (LANE() == 0) { L.cxy[0] = CAND_PACK(r[5], r[6]); L.ccost[64] = 0; L.ccost[128] = 0; }
    prim_eval_list(F, &L, L.fenc, r[2], r[3], r[4], 1, mflag | EV_CHROMA | EV_PROBE, 0, 0);
    if (LANE() == 0) { out[3 * blockIdx.x] = L.ccost[0]; out[3 * blockIdx.x + 1] = L.ccost[64]; out[3 * blockIdx.x + 2] = L.ccost[128]; }
}

/* probe of the RD stage's pixel metrics and intra predictors (SURVEY a3 + the intra SATD analysis of --subme >= 6) on caller-supplied
 * pixels, for parity tests against reference-minted vectors through the C ABI.  One request = 1024 bytes: source macroblock
 * (fenc layout: Y 16x16, then U | V 8x8 side by side, stride 16), a second macroblock in the same layout ("reconstruction"),
 * intra borders top[3][28] ([c][3] = top left, [c][4 + x]) and left[3][16], int32 avail (bit 0 left, bit 1 top) at byte 900.
 * out[32]: 0 ssd of the macroblock without the psy term (x264_pixel_ssd 16x16 + 2 x 8x8, pixel.c:71-96), 1 the same with it
 * (ssd_mb, rdo.c:106-137), 2 / 3 hadamard_ac 16x16 of the second block (pixel.c:306-358; 4x4 / 8x8 energies), 4 / 5 the source's
 * psy-RD energies (x264_mb_cache_fenc_satd, analyse.c:522-549: satd / sa8d sums), 6..9 intra 16x16 costs V, H, DC (the variant avail
 * allows), P (common/predict.c + satd or, at subme 1, sad), 10..13 intra chroma DC, H, V, P over both planes, 14..25 the twelve 4x4
 * modes of block 0 (I4_V .. I4_DC_128); an unavailable mode answers PCAMV_COST_MAX */
static __global__ void __launch_bounds__(64) k_rd_probe(const FrameDev *__restrict__ Fs, const uint8_t *__restrict__ req, int *__restrict__ out)
{
    __shared__ MBLocal L;
    const FrameDev F = Fs[0];
    const int lane = LANE();
    const uint8_t *r = req + 1024 * (size_t)blockIdx.x;
    int *o = out + 32 * blockIdx.x;
    for (int i = lane; i < 96; i += 64) { ((uint32_t *)L.fenc)[i] = ((const uint32_t *)r)[i]; ((uint32_t *)L.pred)[i] = ((const uint32_t *)(r + 384))[i]; }
    for (int i = lane; i < 84; i += 64) ((uint8_t *)L.ib_top)[i] = r[768 + i];
    if (lane < 48) ((uint8_t *)L.ib_left)[lane] = r[852 + lane];
    const int avail = *(const int *)(r + 900);
    if (lane == 0) { L.mb_x = L.mb_y = L.mb_xy = 0; L.neighbour = (avail & 1 ? NB_LEFT : 0) | (avail & 2 ? NB_TOP | NB_TOPRIGHT : 0) | (avail == 3 ? NB_TOPLEFT : 0); }
    PCAMV_WAVE_SYNC();
    FrameDev F0 = F;
    F0.psy_rd = 0;
    const int ssd0 = prim_ssd_mb(F0, &L);
    prim_fenc_complexity(F, &L);
    const int ssd1 = prim_ssd_mb(F, &L);
    int h4, h8;
    prim_hadamard_ac16(L.pred, lane, &h4, &h8);
    if (lane == 0) { o[0] = ssd0; o[1] = ssd1; o[2] = h4; o[3] = h8; o[4] = L.fenc_satd_sum; o[5] = L.fenc_sa8d_sum; }
    prim_intra16_satd(F, &L, avail);
    if (lane < 4) o[6 + lane] = L.ccost[lane];
    PCAMV_WAVE_SYNC();
    prim_intra8c_satd(F, &L, avail);
    if (lane < 4) o[10 + lane] = L.ccost[lane];
    PCAMV_WAVE_SYNC();
    prim_intra4_init(&L);
    if (lane < 12) L.slots[lane] = lane;
    prim_intra4_costs(F, &L, 0, 12, 0);
    if (lane < 12) o[14 + lane] = L.ccost[lane];       /* (every mode is computed on the borders as given: availability is the caller's business) */
}
#endif
