/*
 * check_message_plan.cpp -- TEST-ONLY host build of the control code of k_message_plan (csrc/pcamv_message.h: pcamv_message_run,
 * _run_sum, _run_place, _fold, with a loop over threads standing in for the workgroup and a serial scan for its LDS scan) and of the
 * chain's sibling for planned places (pcamv_extract_chain_slot_at, csrc/pcamv_stc_extract.h).  Built with -fsanitize=address,undefined;
 * every array sits in a heap block of exactly its size.
 *
 * A sequence is a number of calls on one batch: contexts x k jobs of (status, n) each, one emrate, one reservation, a start cursor.
 * It goes through the threaded pieces at 1024 threads (the kernel's) and at 7 (runs of many jobs), then through the chain sibling a
 * context at a time as a lane of k_extract_chain_message does it, and through single steps restated here: every call a loop over its
 * slots, every slot a loop over the contexts, one frame at a time -- pcamv_stc_frame_bits, the host's own matrix builder, one cursor
 * for the batch, one generator per context.  Per job at, m, ok and both column sets, per call the state words, and at the end every
 * context's generator must be equal; the contexts' own PST_RX / PST_OVERRUN / PST_TX must not have moved.
 *
 * usage: check_message_plan <random sequences> ; prints "scripted N" and "sequences N ok N differ 0"
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "stc_mats.h"
#include "pcamv_stc_extract.h"
#include "pcamv_message.h"

#define EOF_CODE (-6)           /* PCAMV_EEOF */
struct Job { int status, n; };
struct Call { int k; std::vector<Job> jobs; };      /* jobs[i * k + w] */
struct Seq { float emrate; long long cap, start; int contexts; std::vector<long long> lcg0; std::vector<Call> calls; };
struct Frame { int m, ok, shorter, longer; long long at; unsigned cs[STC_MAXW], cl[STC_MAXW]; };
struct Want { std::vector<std::vector<Frame>> frames; std::vector<std::vector<long long>> state; std::vector<long long> lcg; };

/* single steps, restated: nothing of pcamv_message.h but the names of the state words */
static void naive(const Seq &q, Want &W)
{
    long long cur = q.start, valid = -1, bad[3] = {-1, -1, -1}, over = 0;
    W.lcg = q.lcg0;
    for (size_t c = 0; c < q.calls.size(); c++) {
        const Call &C = q.calls[c];
        std::vector<Frame> fr(C.jobs.size());
        for (int w = 0; w < C.k; w++)
            for (int i = 0; i < q.contexts; i++) {
                const Job &s = C.jobs[(size_t)i * C.k + w];
                Frame &f = fr[(size_t)i * C.k + w];
                memset(&f, 0, sizeof(f));
                f.at = cur;
                if (s.status == 0) {
                    f.m = pcamv_stc_frame_bits(q.emrate, s.n);
                    if (f.m > 0 && f.m <= s.n) {
                        const double invalpha = (double)s.n / f.m;
                        f.shorter = (int)floor(invalpha); f.longer = (int)ceil(invalpha);
                        f.ok = pcamv_stc_matrix_host(pcamv_stc_mats, f.shorter, PCAMV_STC_HEIGHT, f.cs, &W.lcg[i]) &&
                               pcamv_stc_matrix_host(pcamv_stc_mats, f.longer, PCAMV_STC_HEIGHT, f.cl, &W.lcg[i]);
                    }
                    if (q.cap >= 0 && cur + f.m > q.cap) over = 1;
                    cur += f.m;
                } else if (s.status != EOF_CODE && valid < 0) {
                    valid = cur; bad[0] = (long long)c; bad[1] = w; bad[2] = i;
                }
            }
        W.frames.push_back(fr);
        std::vector<long long> st(MSG_WORDS, 0);
        st[MSG_CURSOR] = cur; st[MSG_VALID] = valid; st[MSG_BAD_CALL] = bad[0]; st[MSG_BAD_SLOT] = bad[1]; st[MSG_BAD_CTX] = bad[2];
        st[MSG_OVERRUN] = over; st[MSG_CALLS] = (long long)c + 1;
        W.state.push_back(st);
    }
}

/* one call through the pieces of k_message_plan with T threads */
static void planned_call(const int *m, const int *status, int contexts, int k, long long cap, long long *state, long long *at, int T)
{
    const long long jobs = (long long)contexts * k;
    long long *sum = (long long *)malloc(T * sizeof(long long)), *fail = (long long *)malloc(T * sizeof(long long));
    for (int t = 0; t < T; t++) {
        long long lo, hi;
        pcamv_message_run(jobs, t, T, &lo, &hi);
        sum[t] = pcamv_message_run_sum(m, status, contexts, k, EOF_CODE, lo, hi, &fail[t]);
    }
    long long total = 0, fail_o = -1;
    for (int t = 0; t < T; t++) { total += sum[t]; if (fail[t] >= 0 && (fail_o < 0 || fail[t] < fail_o)) fail_o = fail[t]; }
    long long before = 0, fail_at = -1;
    int over = 0;
    for (int t = 0; t < T; t++) {
        long long lo, hi, fa = -1;
        pcamv_message_run(jobs, t, T, &lo, &hi);
        over |= pcamv_message_run_place(m, status, contexts, k, cap, lo, hi, state[MSG_CURSOR] + before, fail_o, &fa, at);
        if (fa >= 0) fail_at = fa;
        before += sum[t];
    }
    pcamv_message_fold(state, total, fail_o, fail_at, over, contexts);
    free(sum); free(fail);
}

static int planned(const Seq &q, const Want &W, int T)
{
    int bad = 0;
    long long *state = (long long *)malloc(MSG_WORDS * sizeof(long long));
    long long *pstate = (long long *)malloc((size_t)q.contexts * PST_WORDS * sizeof(long long));
    pcamv_message_state_reset(state, q.start);
    for (int i = 0; i < q.contexts; i++) {
        long long *p = pstate + (size_t)i * PST_WORDS;
        p[PST_TX] = 77; p[PST_RX] = 1000 + i; p[PST_OVERRUN] = 0; p[PST_RX_LCG] = q.lcg0[i];
    }
    for (size_t c = 0; c < q.calls.size(); c++) {
        const Call &C = q.calls[c];
        const size_t jobs = C.jobs.size();
        int *m = (int *)malloc(jobs * sizeof(int)), *status = (int *)malloc(jobs * sizeof(int));
        long long *at = (long long *)malloc(jobs * sizeof(long long)), *at_def = (long long *)malloc(jobs * sizeof(long long));
        long long *state_def = (long long *)malloc(MSG_WORDS * sizeof(long long));
        for (size_t j = 0; j < jobs; j++) { status[j] = C.jobs[j].status; m[j] = status[j] ? 0 : pcamv_stc_frame_bits(q.emrate, C.jobs[j].n); }
        memcpy(state_def, state, MSG_WORDS * sizeof(long long));
        planned_call(m, status, q.contexts, C.k, q.cap, state, at, T);
        pcamv_message_plan(m, status, q.contexts, C.k, q.cap, EOF_CODE, state_def, at_def);       /* the definition agrees with both */
        if (memcmp(state, state_def, MSG_WORDS * sizeof(long long)) || memcmp(at, at_def, jobs * sizeof(long long))) bad = 1;
        for (int w = 0; w < MSG_WORDS; w++) if (state[w] != W.state[c][w]) bad = 1;
        /* the chain, a context at a time in slot order */
        for (int i = 0; i < q.contexts; i++)
            for (int w = 0; w < C.k; w++) {
                const size_t j = (size_t)i * C.k + w;
                int *hdr = (int *)malloc(8 * sizeof(int));
                unsigned *cols = (unsigned *)malloc(2 * STC_MAXW * sizeof(unsigned));
                memset(hdr, 0x5A, 8 * sizeof(int)); memset(cols, 0x5A, 2 * STC_MAXW * sizeof(unsigned));
                hdr[0] = status[j] ? 0 : C.jobs[j].n;
                pcamv_extract_chain_slot_at(pcamv_stc_mats, q.emrate, status[j], at[j], hdr, cols, cols, pstate + (size_t)i * PST_WORDS);
                const Frame &f = W.frames[c][j];
                const long long got = (long long)(((unsigned long long)(unsigned)hdr[7] << 32) | (unsigned)hdr[6]);
                if (got != f.at || hdr[1] != f.m || hdr[2] != f.ok) bad = 1;
                if (f.ok && (memcmp(cols, f.cs, f.shorter * sizeof(unsigned)) || memcmp(cols + STC_MAXW, f.cl, f.longer * sizeof(unsigned)))) bad = 1;
                free(cols); free(hdr);
            }
        free(m); free(status); free(at); free(at_def); free(state_def);
    }
    for (int i = 0; i < q.contexts; i++) {
        const long long *p = pstate + (size_t)i * PST_WORDS;
        if (p[PST_TX] != 77 || p[PST_RX] != 1000 + i || p[PST_OVERRUN] != 0 || p[PST_RX_LCG] != W.lcg[i]) bad = 1;
    }
    free(state); free(pstate);
    return bad;
}

static Seq seq(float emrate, long long cap, long long start, int contexts, std::vector<Call> calls)
{
    Seq q; q.emrate = emrate; q.cap = cap; q.start = start; q.contexts = contexts; q.calls = calls;
    for (int i = 0; i < contexts; i++) q.lcg0.push_back(i % 3 ? 1 + 7919LL * i : 1);
    return q;
}
static Call call(int contexts, int k, int n, std::vector<long long> failed = {}, int code = -1)
{
    Call C; C.k = k; C.jobs.assign((size_t)contexts * k, Job{0, n});
    for (long long o : failed) C.jobs[(size_t)(o % contexts) * k + (size_t)(o / contexts)].status = code;      /* by order index */
    return C;
}

int main(int argc, char **argv)
{
    const int n_random = argc > 1 ? atoi(argv[1]) : 0;
    std::vector<Seq> all;
    /* table widths (0.5), generator widths above 20 (0.04 at n = 72: 36 / 36; 0.03 at 99: 49 / 50): one job, a step, windows, both
     * sides of the run boundaries of 1024 threads (1023 / 1024 / 1025 jobs) */
    for (float e : {0.5f, 0.04f, 0.03f}) {
        const int n = e == 0.03f ? 99 : 72;
        all.push_back(seq(e, -1, 0, 1, {call(1, 1, n)}));
        all.push_back(seq(e, -1, 0, 6, {call(6, 1, n), call(6, 1, n), call(6, 1, n)}));
        all.push_back(seq(e, -1, 5, 3, {call(3, 8, n), call(3, 1, n), call(3, 64, n)}));
        all.push_back(seq(e, -1, 0, 1023, {call(1023, 1, n)}));
        all.push_back(seq(e, -1, 0, 1024, {call(1024, 1, n)}));
        all.push_back(seq(e, -1, 0, 1025, {call(1025, 1, n), call(1025, 2, n)}));
        all.push_back(seq(e, -1, 0, 129, {call(129, 8, n)}));
        /* failed jobs: the first, a middle and the last in order, EEOF among them, several calls with the sticky words */
        for (int code : {-1, -5, -6}) {
            all.push_back(seq(e, -1, 0, 5, {call(5, 3, n, {0}, code)}));
            all.push_back(seq(e, -1, 0, 5, {call(5, 3, n, {7}, code)}));
            all.push_back(seq(e, -1, 0, 5, {call(5, 3, n, {14}, code)}));
            all.push_back(seq(e, -1, 9, 5, {call(5, 3, n), call(5, 3, n, {4, 9}, code), call(5, 3, n, {0}, -1), call(5, 1, n)}));
            all.push_back(seq(e, -1, 0, 4, {call(4, 2, n, {0, 1, 2, 3, 4, 5, 6, 7}, code), call(4, 2, n)}));
        }
    }
    /* n = 0, m = 0, m > n (bits per frame), no sub-matrix for the width */
    all.push_back(seq(0.5f, -1, 0, 4, {call(4, 2, 0), call(4, 2, 72)}));
    all.push_back(seq(0.01f, -1, 0, 4, {call(4, 2, 72)}));
    all.push_back(seq(100.0f, -1, 0, 4, {call(4, 2, 72), call(4, 1, 101)}));
    all.push_back(seq(2.0f, -1, 0, 3, {call(3, 2, 600), call(3, 2, 513), call(3, 1, 72)}));
    all.push_back(seq(35.0f, -1, 0, 6, {call(6, 3, 72)}));
    /* reservations that end before a job, inside one and at its last bit (m = 36); a start cursor above 2^32 */
    all.push_back(seq(0.5f, 36 * 4, 0, 2, {call(2, 2, 72)}));
    all.push_back(seq(0.5f, 36 * 4 - 1, 0, 2, {call(2, 2, 72)}));
    all.push_back(seq(0.5f, 36 * 2 + 10, 0, 2, {call(2, 2, 72), call(2, 1, 72)}));
    all.push_back(seq(0.5f, 36 * 2, 0, 2, {call(2, 1, 72), call(2, 1, 72)}));
    all.push_back(seq(0.5f, -1, (1LL << 32) + 12345, 65, {call(65, 2, 72, {70}, -1), call(65, 1, 72)}));
    all.push_back(seq(0.5f, (1LL << 33) + 100, 1LL << 33, 3, {call(3, 2, 72)}));
    const size_t scripted = all.size();
    /* seeded */
    unsigned long long rng = 0x9E3779B97F4A7C15ULL;
    auto draw = [&rng](unsigned mod) { rng = rng * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)(rng >> 33) % mod; };
    static const float rates[] = {0.5f, 0.04f, 0.03f, 0.01f, 0.1f, 0.3f, 1.0f, 2.0f, 35.0f, 100.0f, 0.049f};
    static const int ns[] = {0, 1, 2, 19, 20, 21, 72, 99, 257, 513, 600, 1584};
    for (int r = 0; r < n_random; r++) {
        const int contexts = r % 11 == 0 ? 1 + (int)draw(1100) : 1 + (int)draw(40), n_calls = 1 + (int)draw(4), fail_in = (int)draw(4);
        Seq q = seq(rates[draw(sizeof(rates) / sizeof(rates[0]))], -1, draw(2) ? 0 : (long long)draw(1u << 31) * (draw(2) ? 1 : 16), contexts, {});
        long long room = 0;
        for (int c = 0; c < n_calls; c++) {
            Call C; C.k = contexts > 64 ? 1 + (int)draw(3) : r % 7 == 0 ? 64 : 1 + (int)draw(9);
            for (int j = 0; j < contexts * C.k; j++) {
                const int st = fail_in && draw(8 * fail_in) == 0 ? -1 - (int)draw(6) : 0;
                C.jobs.push_back(Job{st, draw(4) ? ns[draw(sizeof(ns) / sizeof(ns[0]))] : (int)draw(1600)});
                room += 40;
            }
            q.calls.push_back(C);
        }
        if (draw(3) == 0) q.cap = q.start + draw((unsigned)(room < (1 << 30) ? room : (1 << 30)) + 1);
        all.push_back(q);
    }
    size_t ok = 0, differ = 0;
    for (const Seq &q : all) {
        Want W;
        naive(q, W);
        const int bad = planned(q, W, 1024) | planned(q, W, 7);
        if (bad) { differ++; printf("differs: emrate %g cap %lld start %lld contexts %d calls %zu\n", q.emrate, q.cap, q.start, q.contexts, q.calls.size()); }
        else ok++;
    }
    printf("scripted %zu\n", scripted);
    printf("sequences %zu ok %zu differ %zu\n", all.size(), ok, differ);
    return differ != 0;
}
