/*
 * pcamv_rate.h -- a QP per context on the device, and the library's rate controller: the control code of k_frame_qp and
 * k_rate_update (pcamv_rate.hip.h).
 *
 * Compiles for the device, for the host side of the library (pcamv_gpu_rate_update, the definition without a GPU) and for plain C++
 * test programs (tests/fuzz/check_rate.cpp, with PCAMV_HOST_EMU): no HIP type, no table in memory.
 *
 * The row of a QP is what pcamv_frame_set_qp and the two table pointers write into a frame descriptor: QPROW_DWORDS dwords, built on
 * the host from a descriptor that went through exactly those (qprow_take), put back a dword per lane (qprow_put).  Where the dwords of
 * a row lie in a FrameDev is stated once, in qprow_dst; nothing else of the descriptor is touched.
 *
 * The controller's rule is in pcamv_gpu.h (pcamv_gpu_rate_update); pcamv_rate_step below is its only implementation.
 */
#ifndef PCAMV_RATE_H
#define PCAMV_RATE_H
#include <stddef.h>
#include <stdint.h>
#include "pcamv_common.h"

#if defined(__HIPCC__) && !defined(PCAMV_HOST_EMU)
#define PCAMV_RATE_HD __host__ __device__ static inline
#else
#define PCAMV_RATE_HD static inline
#endif

/* the dwords of a row: cost_mv (2), qp chroma_qp lambda (3), q_mf q_bias dq_mf dq_mf_c lambda2_chroma (19), lambda2 (1),
 * q_mf_i q_bias_i (6), cabac_init (2) */
#define QPROW_DWORDS 33
#define QPROW_QPS 52
static_assert(sizeof(FrameDev) % 4 == 0 && sizeof(void *) == 8, "a descriptor is patched by dwords, a pointer is two of them");
static_assert(offsetof(FrameDev, cost_mv) % 8 == 0 && offsetof(FrameDev, cabac_init) % 8 == 0, "the two table pointers");
static_assert(offsetof(FrameDev, chroma_qp) == offsetof(FrameDev, qp) + 4 && offsetof(FrameDev, lambda) == offsetof(FrameDev, qp) + 8, "qp, chroma_qp, lambda lie together");
static_assert(offsetof(FrameDev, q_bias) == offsetof(FrameDev, q_mf) + 24 && offsetof(FrameDev, dq_mf) == offsetof(FrameDev, q_mf) + 48 &&
              offsetof(FrameDev, dq_mf_c) == offsetof(FrameDev, q_mf) + 60 && offsetof(FrameDev, lambda2_chroma) == offsetof(FrameDev, q_mf) + 72,
              "the inter quantiser sets and lambda2_chroma lie together");
static_assert(offsetof(FrameDev, q_bias_i) == offsetof(FrameDev, q_mf_i) + 12, "the intra quantiser set lies together");

/* dword l of a row is dword qprow_dst(l) of a FrameDev */
PCAMV_RATE_HD int qprow_dst(int l)
{
    if (l < 2) return (int)(offsetof(FrameDev, cost_mv) / 4) + l;
    if (l < 5) return (int)(offsetof(FrameDev, qp) / 4) + l - 2;
    if (l < 24) return (int)(offsetof(FrameDev, q_mf) / 4) + l - 5;
    if (l < 25) return (int)(offsetof(FrameDev, lambda2) / 4);
    if (l < 31) return (int)(offsetof(FrameDev, q_mf_i) / 4) + l - 25;
    return (int)(offsetof(FrameDev, cabac_init) / 4) + l - 31;
}
/* a QP as it may index a table: (clamped, was it outside 0 .. 51) */
PCAMV_RATE_HD int qprow_clamp(int qp, int *outside)
{
    *outside = qp < 0 || qp >= QPROW_QPS;
    return qp < 0 ? 0 : qp >= QPROW_QPS ? QPROW_QPS - 1 : qp;
}
/* host: the row out of a descriptor pcamv_frame_set_qp and the table pointers were written into */
static inline void qprow_take(const FrameDev *F, uint32_t *row)
{
    const uint32_t *w = (const uint32_t *)(const void *)F;
    for (int l = 0; l < QPROW_DWORDS; l++) row[l] = w[qprow_dst(l)];
}
/* lane l's share of the patch: the context's QP as it stands in its cell (any int32), the 52 rows of its table, its descriptor */
PCAMV_RATE_HD void qprow_put(uint32_t *desc, const uint32_t *rows, int qp, int l)
{
    int outside;
    const int q = qprow_clamp(qp, &outside);
    if (l >= 0 && l < QPROW_DWORDS) desc[qprow_dst(l)] = rows[q * QPROW_DWORDS + l];
}

/* ---- the controller (pcamv_gpu.h: the rule) */
#define RATE_DEBT_MAX (1LL << 40)
#define RATE_LEN_MAX (1LL << 41)        /* bytes of one picture the rule tells apart */
PCAMV_RATE_HD int pcamv_rate_params_ok(const pcamv_rate_params_t *p)
{
    return p->target_bits >= 1 && p->target_bits <= RATE_DEBT_MAX && p->qp_min >= 0 && p->qp_max <= 51 && p->qp_min <= p->qp_init && p->qp_init <= p->qp_max &&
           p->max_step >= 1 && p->max_step <= 6 && p->window >= 1 && p->window <= 1024;
}
PCAMV_RATE_HD void pcamv_rate_open(const pcamv_rate_params_t *p, pcamv_rate_state_t *s, long long len)
{
    s->debt = 0; s->last_len = len; s->pictures = 0; s->qp = p->qp_init; s->last_d = 0;
}
/* one picture: the stream's length behind it and its write status; returns d */
PCAMV_RATE_HD int pcamv_rate_step(const pcamv_rate_params_t *p, pcamv_rate_state_t *s, long long len, int write_status)
{
    const long long P0 = 65536;
    const long long T = p->target_bits;
    long long bytes = len - s->last_len;
    bytes = bytes < 0 ? 0 : bytes > RATE_LEN_MAX ? RATE_LEN_MAX : bytes;
    const long long bits = 8 * bytes;
    s->last_len = len;
    int d;
    if (write_status != 0) d = p->max_step;
    else {
        long long debt = s->debt + bits - T;
        debt = debt > RATE_DEBT_MAX ? RATE_DEBT_MAX : debt < -RATE_DEBT_MAX ? -RATE_DEBT_MAX : debt;
        s->debt = debt;
        long long want = T - debt / p->window;
        if (want < T / 4) want = T / 4;
        if (want < 1) want = 1;
        d = 0;
        for (int k = 1; k <= p->max_step; k++) {
            /* 2^(k/6) in Q16 */
            const long long Pk = k == 1 ? 73562 : k == 2 ? 82570 : k == 3 ? 92682 : k == 4 ? 104032 : k == 5 ? 116772 : 131072;
            if (bits >= want) { if (bits * P0 >= want * Pk) d = k; }
            else if (bits == 0 || want * P0 >= bits * Pk) d = -k;
        }
    }
    int qp = s->qp + d;
    qp = qp < p->qp_min ? p->qp_min : qp > p->qp_max ? p->qp_max : qp;
    s->qp = qp; s->last_d = d; s->pictures++;
    return d;
}
#endif
