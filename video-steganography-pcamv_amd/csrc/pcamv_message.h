/*
 * pcamv_message.h -- one message for a batch: which bits of it every frame of every context takes.
 *
 * Compiles for the device (k_message_plan, pcamv_message.hip.h), for the host side of the library (pcamv_gpu_message_plan, the
 * definition without a GPU) and for plain C++ test programs (tests/fuzz/check_message_plan.cpp): no HIP type, no table.
 *
 * A job is one frame of one context in one call: a step call has k = 1 slot per context, a window call k.  The arrays of a call are
 * context-major as the window's are (job j = i * k + w is slot w of context i); the ORDER of the jobs is slot-major, context-minor:
 * order index o = w * contexts + i, so that a window of k is observationally k steps.  With the batch cursor B at the start of a call
 *
 *     at(o) = B + sum of bits(o') over o' < o,        B += sum of bits(o) over all jobs of the call
 *
 * bits = the frame's m (pcamv_stc_frame_bits of its carrier count) for a job of status 0 -- whatever stc_ok or the sub-matrices turn
 * out to be, the per-context rule --, 0 for every other status.  The status `eof` (PCAMV_EEOF: the context's stream has no further
 * unit) is no failure; any other non-zero status is one: its m is unknown, so everything behind it is misaligned.  The state keeps,
 * sticky until it is reset, the smallest `at` of a failed job (MSG_VALID; -1 while there is none) and that job's (call number since
 * the reset, slot, context).  A job of status 0 that ends beyond the capacity sets MSG_OVERRUN (the rule of a context's received
 * stream: its bits at or beyond the capacity are dropped by k_extract_bits, never written).
 */
#ifndef PCAMV_MESSAGE_H
#define PCAMV_MESSAGE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define PCAMV_MSG_HD __host__ __device__ static inline
#else
#define PCAMV_MSG_HD static inline
#endif

/* the words of a batch's message state (device memory; the host definition keeps the same) */
enum { MSG_CURSOR = 0,        /* B: message bits handed out (sender) / counted in the stream (receiver) so far */
       MSG_VALID = 1,         /* the smallest `at` of a failed job, -1: none so far */
       MSG_BAD_CALL = 2,      /* that job: calls planned since the reset before its own, */
       MSG_BAD_SLOT = 3,      /* ... its slot w */
       MSG_BAD_CTX = 4,       /* ... its context i (all three -1 while there is none) */
       MSG_OVERRUN = 5,       /* != 0: a job ended beyond the capacity */
       MSG_CALLS = 6,         /* calls planned since the reset */
       MSG_WORDS = 8 };
#define PCAMV_MSG_NO_CAP (-1LL)         /* capacity of a plan nothing bounds (the sender's) */

PCAMV_MSG_HD void pcamv_message_state_reset(long long *state, long long cursor)
{
    for (int i = 0; i < MSG_WORDS; i++) state[i] = 0;
    state[MSG_CURSOR] = cursor;
    state[MSG_VALID] = state[MSG_BAD_CALL] = state[MSG_BAD_SLOT] = state[MSG_BAD_CTX] = -1;
}
/* what a job contributes, and whether it is a failure */
PCAMV_MSG_HD long long pcamv_message_job_bits(int m, int status) { return status == 0 && m > 0 ? (long long)m : 0; }
PCAMV_MSG_HD int pcamv_message_job_failed(int status, int eof) { return status != 0 && status != eof; }
/* the job (its place in the call's arrays) of order index o */
PCAMV_MSG_HD long long pcamv_message_job_of(long long o, int contexts, int k) { return (o % contexts) * (long long)k + o / contexts; }

/* ---- the definition: one walk over the jobs in order.  m / status: [contexts * k] (status NULL: all 0); at: [contexts * k] out */
PCAMV_MSG_HD void pcamv_message_plan(const int *m, const int *status, int contexts, int k, long long cap, int eof, long long *state, long long *at)
{
    long long cur = state[MSG_CURSOR];
    for (int w = 0; w < k; w++)
        for (int i = 0; i < contexts; i++) {
            const long long j = (long long)i * k + w;
            const int st = status ? status[j] : 0;
            const long long bits = pcamv_message_job_bits(m[j], st);
            at[j] = cur;
            if (pcamv_message_job_failed(st, eof) && state[MSG_VALID] < 0) {
                state[MSG_VALID] = cur; state[MSG_BAD_CALL] = state[MSG_CALLS]; state[MSG_BAD_SLOT] = w; state[MSG_BAD_CTX] = i;
            }
            if (st == 0 && cap >= 0 && cur + bits > cap) state[MSG_OVERRUN] = 1;
            cur += bits;
        }
    state[MSG_CURSOR] = cur;
    state[MSG_CALLS] += 1;
}

/* ---- the same in the pieces k_message_plan is made of: T threads, thread t takes the run [lo, hi) of order indices; between the
 * pieces the workgroup scans the runs' sums and takes the minimum of their first failures (a loop over t in a test program) */
PCAMV_MSG_HD void pcamv_message_run(long long jobs, int t, int T, long long *lo, long long *hi)
{
    const long long chunk = (jobs + T - 1) / T, a = (long long)t * chunk;
    *lo = a < jobs ? a : jobs;
    *hi = *lo + chunk < jobs ? *lo + chunk : jobs;
}
/* first piece: the bits of the run; *first_fail = order index of its first failed job, or -1 */
PCAMV_MSG_HD long long pcamv_message_run_sum(const int *m, const int *status, int contexts, int k, int eof, long long lo, long long hi, long long *first_fail)
{
    long long sum = 0;
    *first_fail = -1;
    for (long long o = lo; o < hi; o++) {
        const long long j = pcamv_message_job_of(o, contexts, k);
        const int st = status ? status[j] : 0;
        sum += pcamv_message_job_bits(m[j], st);
        if (*first_fail < 0 && pcamv_message_job_failed(st, eof)) *first_fail = o;
    }
    return sum;
}
/* second piece: every job's `at` from the bits in front of the run (`base`, cursor included); returns whether a job of the run ended
 * beyond the capacity; the thread whose run holds order index fail_o leaves that job's `at` in *fail_at */
PCAMV_MSG_HD int pcamv_message_run_place(const int *m, const int *status, int contexts, int k, long long cap, long long lo, long long hi, long long base,
                                         long long fail_o, long long *fail_at, long long *at)
{
    int overrun = 0;
    for (long long o = lo; o < hi; o++) {
        const long long j = pcamv_message_job_of(o, contexts, k);
        const int st = status ? status[j] : 0;
        const long long bits = pcamv_message_job_bits(m[j], st);
        at[j] = base;
        if (o == fail_o) *fail_at = base;
        if (st == 0 && cap >= 0 && base + bits > cap) overrun = 1;
        base += bits;
    }
    return overrun;
}
/* last piece, one thread: the call's total, its first failure (fail_o < 0: none) and the overrun folded into the state */
PCAMV_MSG_HD void pcamv_message_fold(long long *state, long long total, long long fail_o, long long fail_at, int overrun, int contexts)
{
    if (fail_o >= 0 && state[MSG_VALID] < 0) {
        state[MSG_VALID] = fail_at; state[MSG_BAD_CALL] = state[MSG_CALLS]; state[MSG_BAD_SLOT] = fail_o / contexts; state[MSG_BAD_CTX] = fail_o % contexts;
    }
    if (overrun) state[MSG_OVERRUN] = 1;
    state[MSG_CURSOR] += total;
    state[MSG_CALLS] += 1;
}
#endif
