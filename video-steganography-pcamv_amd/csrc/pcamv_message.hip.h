/*
 * pcamv_message.hip.h -- one message for a batch (gfx950), launched by pcamv_gpu.hip only; included behind pcamv_embed.hip.h.
 *
 *   k_message_count          sender: per context of a step its carrier count as k_embed_prepare will find it, then m
 *   k_message_jobs           receiver: per job (m, status) out of the descriptors, behind k_extract_count
 *   k_message_plan           the rule of pcamv_message.h over the jobs of a call: every job's `at`, the batch's state
 *   k_extract_chain_message  k_extract_chain with the planned `at`
 *   k_message_check / k_message_check_sum   bits in which the batch's received stream differs from the attached message
 */
#ifndef PCAMV_MESSAGE_HIP_H
#define PCAMV_MESSAGE_HIP_H
#include "pcamv_embed.hip.h"
#include "pcamv_message.h"

#define MSG_PLAN_THREADS 1024

/* One workgroup per context: n exactly as dev_carrier_scan<false> sums it (carrier_slots of every record), then m.  One thread per
 * record, 256 apart: of a record's 236 bytes the first 16 (type, partition, sub-partitions) and the last 4 (used) are asked for, so a
 * wave's loads touch the first and the last 64 bytes of each record and leave the motion and cost arrays between them alone. */
static __global__ void __launch_bounds__(256) k_message_count(const EmbedDev *__restrict__ Es, int *__restrict__ m_out)
{
    const pcamv_mb_t *__restrict__ mbs = Es[blockIdx.x].mbs;
    const int n_mb = Es[blockIdx.x].n_mb, t = threadIdx.x;
    __shared__ int s_sum[4];
    int cnt = 0, slots[16];
    for (int xy = t; xy < n_mb; xy += 256) {
        const pcamv_mb_t *mb = &mbs[xy];
        cnt += carrier_slots(mb->i_type, mb->i_partition, mb->i_sub_partition, mb->used, slots);
    }
    cnt = wave_sum_all(cnt);
    if ((t & 63) == 0) s_sum[t >> 6] = cnt;
    __syncthreads();
    if (t == 0) m_out[blockIdx.x] = pcamv_stc_frame_bits(Es[blockIdx.x].emrate, s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]);
}

/* One thread per job, behind k_extract_count (hdr[0] = n): the job's m and its status.  first (optional): the code of the first stage
 * of a stream call that failed, which k_stream_status puts in the parser's place only after the receiver's kernels */
static __global__ void __launch_bounds__(256) k_message_jobs(const ExtractDev *__restrict__ Xs, const int *__restrict__ first, int jobs,
                                                            int *__restrict__ m_out, int *__restrict__ status_out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= jobs) return;
    const int *ss = Xs[j].slice_status;
    const int st = first && first[j] ? first[j] : ss ? *ss : 0;
    m_out[j] = st ? 0 : pcamv_stc_frame_bits(Xs[j].emrate, Xs[j].hdr[0]);
    status_out[j] = st;
}

/* The plan of one call, one workgroup: two levels.  Thread t sums the run of order indices pcamv_message_run gives it (at most 256 at
 * 4096 contexts x 64 slots), the 1024 sums are scanned in LDS, then every thread walks its run again and writes the jobs' `at`.  The
 * first failed job is the minimum of the runs' first failures.  One launch, nothing read by the host; the next launch on the stream
 * is what waits for it.  tx (optional, k == 1): the sender's contexts, whose pstate[PST_TX] gets the job's `at` -- where
 * k_embed_prepare reads its cursor. */
static __global__ void __launch_bounds__(MSG_PLAN_THREADS) k_message_plan(const int *__restrict__ m, const int *__restrict__ status, int contexts, int k,
                                                                          long long cap, long long *__restrict__ state, long long *__restrict__ at,
                                                                          const EmbedDev *__restrict__ tx)
{
    __shared__ long long s_sum[MSG_PLAN_THREADS], s_fail[MSG_PLAN_THREADS];
    __shared__ long long s_fail_at;
    __shared__ int s_over;
    const int t = threadIdx.x;
    const long long jobs = (long long)contexts * k;
    long long lo, hi, fail;
    pcamv_message_run(jobs, t, MSG_PLAN_THREADS, &lo, &hi);
    const long long own = pcamv_message_run_sum(m, status, contexts, k, PCAMV_EEOF, lo, hi, &fail);
    s_sum[t] = own; s_fail[t] = fail < 0 ? 0x7fffffffffffffffLL : fail;
    if (t == 0) { s_fail_at = -1; s_over = 0; }
    __syncthreads();
    for (int off = 1; off < MSG_PLAN_THREADS; off <<= 1) {      /* inclusive Hillis-Steele scan of the sums, running minimum of the failures */
        const long long v = t >= off ? s_sum[t - off] : 0, f = t >= off ? s_fail[t - off] : 0x7fffffffffffffffLL;
        __syncthreads();
        s_sum[t] += v; s_fail[t] = f < s_fail[t] ? f : s_fail[t];
        __syncthreads();
    }
    const long long total = s_sum[MSG_PLAN_THREADS - 1], fail_min = s_fail[MSG_PLAN_THREADS - 1];
    const long long fail_o = fail_min == 0x7fffffffffffffffLL ? -1 : fail_min;
    const long long base = state[MSG_CURSOR] + s_sum[t] - own;
    long long fail_at = -1;
    const int over = pcamv_message_run_place(m, status, contexts, k, cap, lo, hi, base, fail_o, &fail_at, at);
    if (fail_at >= 0) s_fail_at = fail_at;          /* (one thread's run holds fail_o) */
    if (over) s_over = 1;
    if (tx) for (long long o = lo; o < hi; o++) tx[o].pstate[PST_TX] = at[o];       /* k == 1: job = order index = context */
    __syncthreads();                                /* every thread has read the cursor */
    if (t == 0) pcamv_message_fold(state, total, fail_o, s_fail_at, s_over, contexts);
}

/* k_extract_chain with the planned `at`: one lane per context, its k slots in slot order through the sibling of pcamv_extract_chain_slot */
static __global__ void __launch_bounds__(64) k_extract_chain_message(const ExtractDev *__restrict__ Xs, int n, int k, const int *__restrict__ status,
                                                                     const long long *__restrict__ at)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    for (int w = 0; w < k; w++) {
        const long long j = (long long)i * k + w;
        const ExtractDev &X = Xs[j];
        pcamv_extract_chain_slot_at(pcamv_stc_mats_dev, X.emrate, status[j], at[j], X.hdr, X.cols, X.cols, X.pstate);
    }
}

/* Bits in which the received stream differs from the message over [0, min(received, reserved)), message bits past its end counting as
 * zeros: every workgroup takes bytes 256 apart over the grid and leaves one partial, k_message_check_sum adds them up. */
#define MSG_CHECK_GROUPS 1024
static __global__ void __launch_bounds__(256) k_message_check(const uint8_t *__restrict__ rx, long long cap_bits, const long long *__restrict__ state,
                                                             const uint8_t *__restrict__ msg, long long msg_bits, long long *__restrict__ partial)
{
    __shared__ int s_sum[4];
    const int t = threadIdx.x;
    long long got = state[MSG_CURSOR];
    if (got > cap_bits) got = cap_bits;
    const long long nbytes = (got + 7) >> 3, pbytes = msg ? (msg_bits + 7) >> 3 : 0;
    long long diff = 0;
    for (long long b = (long long)blockIdx.x * 256 + t; b < nbytes; b += (long long)gridDim.x * 256) {
        unsigned p = b < pbytes ? msg[b] : 0u;
        if (b == pbytes - 1 && (msg_bits & 7)) p &= 0xff00u >> (msg_bits & 7);          /* what the caller's last byte holds beyond the message */
        unsigned d = rx[b] ^ p;
        if (b == nbytes - 1 && (got & 7)) d &= 0xff00u >> (got & 7);
        diff += __popc(d & 0xffu);
    }
    const int d32 = wave_sum_all((int)diff);        /* (a wave's count fits: 2^31 differing bits in one wave's share need a stream of terabytes) */
    if ((t & 63) == 0) s_sum[t >> 6] = d32;
    __syncthreads();
    if (t == 0) partial[blockIdx.x] = (long long)s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}
static __global__ void __launch_bounds__(256) k_message_check_sum(const long long *__restrict__ partial, int groups, long long *__restrict__ out)
{
    __shared__ long long s_sum[256];
    const int t = threadIdx.x;
    long long v = 0;
    for (int g = t; g < groups; g += 256) v += partial[g];
    s_sum[t] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) s_sum[t] += s_sum[t + off];
        __syncthreads();
    }
    if (t == 0) *out = s_sum[0];
}
#endif
