/*
 * check_extract_window.cpp -- TEST-ONLY host build of what chains from frame to frame on the receiving side
 * (pcamv_extract_chain_slot, csrc/pcamv_stc_extract.h): the function thread 64 of k_extract_prepare runs for its one frame and a lane of
 * k_extract_chain runs for the k slots of a window.  Built with -fsanitize=address,undefined; every slot's hdr and cols sit in heap
 * blocks of exactly their size.
 *
 * A sequence is k slots of (status, n) at one emrate and one reservation.  It goes through the chain function in both forms -- the
 * window's (columns built in place) and the step's (built in a work array, copied once both stand) -- and through a naive walk
 * written out here, one frame at a time the way k single steps go: pcamv_stc_frame_bits, the host's own matrix builder
 * (pcamv_stc_matrix_host), a cursor, a generator state, a flag.  Per slot m, ok, at and both column sets, and at the end cursor,
 * generator state and overrun flag must be equal.
 *
 * usage: check_extract_window <random sequences> ; prints "sequences N ok N differ 0"
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "stc_mats.h"
#include "pcamv_stc_extract.h"

struct Slot { int status, n; };
struct Seq { float emrate; long long cap_bits, at0, lcg0; std::vector<Slot> slots; };
struct Frame { int m, ok, shorter, longer; long long at; unsigned cs[STC_MAXW], cl[STC_MAXW]; };

/* k single steps, restated */
static void naive(const Seq &q, std::vector<Frame> &out, long long *rx, long long *lcg, long long *overrun)
{
    *rx = q.at0; *lcg = q.lcg0; *overrun = 0;
    for (const Slot &s : q.slots) {
        Frame f;
        memset(&f, 0, sizeof(f));
        f.at = *rx;
        if (!s.status) {
            f.m = pcamv_stc_frame_bits(q.emrate, s.n);
            if (f.m > 0 && f.m <= s.n) {
                const double invalpha = (double)s.n / f.m;
                f.shorter = (int)floor(invalpha); f.longer = (int)ceil(invalpha);
                f.ok = pcamv_stc_matrix_host(pcamv_stc_mats, f.shorter, PCAMV_STC_HEIGHT, f.cs, lcg) &&
                       pcamv_stc_matrix_host(pcamv_stc_mats, f.longer, PCAMV_STC_HEIGHT, f.cl, lcg);
            }
            *rx += f.m;
            if (*rx > q.cap_bits) *overrun = 1;
        }
        out.push_back(f);
    }
}

/* the chain function over the slots; in_place: the window's form, else the step's */
static int chained(const Seq &q, const std::vector<Frame> &want, long long rx, long long lcg, long long overrun, int in_place)
{
    long long *pstate = (long long *)malloc(PST_WORDS * sizeof(long long));
    pstate[PST_TX] = 77; pstate[PST_RX] = q.at0; pstate[PST_OVERRUN] = 0; pstate[PST_RX_LCG] = q.lcg0;
    int bad = 0;
    for (size_t w = 0; w < q.slots.size(); w++) {
        int *hdr = (int *)malloc(8 * sizeof(int));
        unsigned *cols = (unsigned *)malloc(2 * STC_MAXW * sizeof(unsigned)), *work = in_place ? cols : (unsigned *)malloc(2 * STC_MAXW * sizeof(unsigned));
        memset(hdr, 0x5A, 8 * sizeof(int)); memset(cols, 0x5A, 2 * STC_MAXW * sizeof(unsigned));
        const Slot &s = q.slots[w];
        hdr[0] = s.status ? 0 : s.n;            /* (k_extract_count; k_extract_prepare's own thread) */
        pcamv_extract_chain_slot(pcamv_stc_mats, q.emrate, s.status, 1, q.cap_bits, hdr, work, cols, pstate);
        const Frame &f = want[w];
        const long long at = (long long)(((unsigned long long)(unsigned)hdr[7] << 32) | (unsigned)hdr[6]);
        if (hdr[0] != (s.status ? 0 : s.n) || hdr[1] != f.m || hdr[2] != f.ok || at != f.at) bad = 1;
        if (f.ok && (memcmp(cols, f.cs, f.shorter * sizeof(unsigned)) || memcmp(cols + STC_MAXW, f.cl, f.longer * sizeof(unsigned)))) bad = 1;
        if (!in_place) free(work);
        free(cols); free(hdr);
    }
    if (pstate[PST_TX] != 77 || pstate[PST_RX] != rx || pstate[PST_RX_LCG] != lcg || pstate[PST_OVERRUN] != overrun) bad = 1;
    free(pstate);
    return bad;
}

static Seq seq(float emrate, long long cap, std::vector<Slot> slots, long long at0 = 0, long long lcg0 = 1)
{
    Seq q; q.emrate = emrate; q.cap_bits = cap; q.at0 = at0; q.lcg0 = lcg0; q.slots = slots;
    return q;
}
static std::vector<Slot> same(int k, int n, int status = 0) { return std::vector<Slot>(k, Slot{status, n}); }
static std::vector<Slot> failing(int k, int n, std::vector<int> where, int code)
{
    std::vector<Slot> v = same(k, n);
    for (int w : where) v[w].status = code;
    return v;
}

int main(int argc, char **argv)
{
    const int n_random = argc > 1 ? atoi(argv[1]) : 0;
    const long long big = 1LL << 40;
    std::vector<Seq> all;
    /* one slot and the most a window holds, widths inside the table (emrate 0.5) and from the generator (0.04 at n = 72: widths 36 / 36) */
    for (float e : {0.5f, 0.04f}) {
        all.push_back(seq(e, big, same(1, 72)));
        all.push_back(seq(e, big, same(64, 72)));
        all.push_back(seq(e, big, same(64, 99), 12345, 987654321));
        /* failed slots at the first, a middle and the last place, several, and all */
        for (int code : {-1, -5, -6}) {
            all.push_back(seq(e, big, failing(5, 72, {0}, code)));
            all.push_back(seq(e, big, failing(5, 72, {2}, code)));
            all.push_back(seq(e, big, failing(5, 72, {4}, code)));
            all.push_back(seq(e, big, failing(7, 72, {0, 3, 4, 6}, code), 31));
            all.push_back(seq(e, big, same(6, 72, code), 5));
        }
    }
    /* n = 0; m = 0 (0.01 * 72 < 1); both among frames that carry */
    all.push_back(seq(0.5f, big, same(3, 0)));
    all.push_back(seq(0.01f, big, same(4, 72)));
    all.push_back(seq(0.5f, big, {{0, 72}, {0, 0}, {0, 1}, {0, 72}}));
    all.push_back(seq(0.01f, big, {{0, 72}, {0, 1584}, {0, 72}}));
    /* emrate above 1 is bits per frame: m > n appends m zero bits; n / m above 256 has no sub-matrix (600 / 2: neither width; 513 / 2:
     * the shorter one is drawn, the longer one cannot be built, and the generator has moved) */
    all.push_back(seq(100.0f, big, {{0, 72}, {0, 99}, {0, 100}, {0, 101}, {0, 72}}));
    all.push_back(seq(2.0f, big, {{0, 72}, {0, 600}, {0, 72}}));
    all.push_back(seq(2.0f, big, {{0, 513}, {0, 512}, {0, 513}, {0, 99}}));
    all.push_back(seq(2.0f, big, {{0, 1}, {0, 2}, {0, 3}}));
    /* widths at the table's edges: 72 / 3 = 24, 72 / 36 = 2, 60 / 3 = 20, 63 / 3 = 21, 40 / 39: 1 and 2 */
    all.push_back(seq(3.0f, big, {{0, 72}, {0, 60}, {0, 63}, {0, 62}}));
    all.push_back(seq(39.0f, big, {{0, 40}, {0, 39}, {0, 78}}));
    /* a reservation that ends inside a slot (m = 36 a frame: inside the third), exactly at a slot's end, and before the first bit */
    all.push_back(seq(0.5f, 36 * 2 + 10, same(4, 72)));
    all.push_back(seq(0.5f, 36 * 2, same(2, 72)));
    all.push_back(seq(0.5f, 36 * 2, same(3, 72)));
    all.push_back(seq(0.5f, 100 + 36, same(2, 72), 100));
    all.push_back(seq(0.04f, 3, failing(4, 72, {1}, -1)));
    const size_t scripted = all.size();
    /* seeded */
    unsigned long long rng = 0x9E3779B97F4A7C15ULL;
    auto draw = [&rng](unsigned mod) { rng = rng * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)(rng >> 33) % mod; };
    static const float rates[] = {0.5f, 0.04f, 0.01f, 0.1f, 0.25f, 0.9f, 1.0f, 2.0f, 7.0f, 100.0f, 0.049f, 0.051f};
    static const int ns[] = {0, 1, 2, 19, 20, 21, 72, 99, 257, 512, 513, 600, 1584};
    for (int r = 0; r < n_random; r++) {
        Seq q;
        q.emrate = rates[draw(sizeof(rates) / sizeof(rates[0]))];
        const int k = r % 7 == 0 ? 64 : 1 + (int)draw(64), fail_in = (int)draw(5);
        for (int w = 0; w < k; w++) {
            const int st = fail_in && draw(fail_in + 1) == 0 ? -1 - (int)draw(6) : 0;
            q.slots.push_back(Slot{st, draw(4) ? ns[draw(sizeof(ns) / sizeof(ns[0]))] : (int)draw(1600)});
        }
        q.at0 = draw(2) ? draw(5000) : 0; q.lcg0 = draw(2) ? 1 : (long long)draw(1u << 31);
        q.cap_bits = draw(3) ? big : q.at0 + draw(40 * k + 1);
        all.push_back(q);
    }
    size_t ok = 0, differ = 0;
    for (const Seq &q : all) {
        std::vector<Frame> want;
        long long rx, lcg, overrun;
        naive(q, want, &rx, &lcg, &overrun);
        const int bad = chained(q, want, rx, lcg, overrun, 1) | chained(q, want, rx, lcg, overrun, 0);
        if (bad) { differ++; printf("differs: emrate %g cap %lld k %zu at %lld\n", q.emrate, q.cap_bits, q.slots.size(), q.at0); }
        else ok++;
    }
    printf("scripted %zu\n", scripted);
    printf("sequences %zu ok %zu differ %zu\n", all.size(), ok, differ);
    return differ != 0;
}
