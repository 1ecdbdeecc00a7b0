/* The control code of one video of many chains (csrc/pcamv_video.h: k_video_cut, k_stream_copy_plan, k_stream_copy, k_stream_join,
 * k_stream_open_heads) under AddressSanitizer + UBSan on the CPU, with the host form of SP_LANES.
 *
 * The cut: every video is run with its bytes in an exact-size heap block at each of the four alignments mod 4 (the block begins 0 .. 3
 * bytes before the video and ends with it), through the index control code as the library drives it -- scans and prefix without a table
 * for the count, then prefix and placing scans over the kept summaries into a table of exactly that many units; the prefix also in the
 * two levels a long stream's index makes it in (vp_local, si_prefix over the blocks, vp_apply), which must leave the same -- and through vg_cut with
 * a table of GOPs of exactly `cap` entries (the case's, else the full count) and working memory of exact size.  The GOP table, the count
 * and the preamble must equal pcamv_gpu_annexb_gops' (csrc/pcamv_mvsyntax.h).  The alignments take turns with where the GOPs go besides:
 * to three contexts from GOP 0 or from GOP 1 on, whose (off, len) must be the GOPs' or (0, 0) past the last.
 *
 * The copy: every job with source and destination in heap blocks that end with the job, at the case's two alignments, must equal memcpy
 * and leave the bytes in front of the destination alone; then all jobs at once, sources in one exact-size block and destinations in
 * another, through vc_plan and vc_job_of as a launch runs them (more than 64 jobs: every lane's share of the prefix).  vj_join and
 * vj_head are run on 70 contexts against their definitions restated.  Built and run by tests/test_video_cpu.py.
 *
 * usage: check_video <cases.bin>      (the file: tests/video_cases.py, write_cases)
 * prints "videos <n> ok <n> differ <n>", "copies <n> ok <n> differ <n>", "joins <n> ok <n> differ <n>"; exit status 1 on any difference. */
#define PCAMV_HOST_EMU 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pcamv_host_tables.h"
#include "pcamv_mvsyntax.h"
#include "pcamv_video.h"

static long n_videos, n_vdiffer, n_copies, n_cdiffer, n_joins, n_jdiffer;

template <class T> static T *exact(size_t n) { return (T *)malloc(n * sizeof(T) ? n * sizeof(T) : 1); }

static int cut_one(const uint8_t *src, long long len, long long cap, const std::vector<pcamv_gop_t> &want, long long want_n, long long want_pre, long long first, int n_ctx)
{
    SiWork work = {exact<uint32_t>(SI_WIN_DWORDS), exact<SiChunk>(64)};
    const long long n_chunks = si_chunks(src, len);
    SiChunk *ch = exact<SiChunk>((size_t)n_chunks), *keep = exact<SiChunk>((size_t)n_chunks);
    unsigned long long longest = 0;
    const SiTable none = {NULL, 0, 1, &longest, 0};
    long long nu = -7, ns = -7;
    for (long long c = 0; c < n_chunks; c++) si_scan(work, src, len, c, 0, ch + c, none);
    if (n_chunks) memcpy(keep, ch, (size_t)n_chunks * sizeof(SiChunk));
    si_prefix(work, src, len, ch, n_chunks, none, &nu, &ns);
    pcamv_unit_t *units = exact<pcamv_unit_t>((size_t)nu);
    const SiTable all = {units, nu, 1, &longest, 0};
    if (n_chunks) memcpy(ch, keep, (size_t)n_chunks * sizeof(SiChunk));
    si_prefix(work, src, len, ch, n_chunks, all, &nu, &ns);
    /* the same prefix in two levels, as a long stream's index makes it: chunk by chunk and count by count what the one wavefront made */
    const long long n_blocks = (n_chunks + VP_BLOCK - 1) / VP_BLOCK;
    SiChunk *B = exact<SiChunk>((size_t)n_blocks);
    pcamv_unit_t *units2 = exact<pcamv_unit_t>((size_t)nu);
    memset((void *)units2, 0x5A, (size_t)nu * sizeof(pcamv_unit_t));
    const SiTable all2 = {units2, nu, 1, &longest, 0};
    long long nu2 = -7, ns2 = -7;
    for (long long blk = 0; blk < n_blocks; blk++) vp_local(work, src, len, keep, n_chunks, blk, B);
    si_prefix(work, src, len, B, n_blocks, all2, &nu2, &ns2);
    for (long long i = 0; i < (n_chunks + 63) / 64 * 64; i++) vp_apply(keep, n_chunks, B, i);
    int two_level_differs = nu2 != nu || ns2 != ns || (n_chunks && memcmp(keep, ch, (size_t)n_chunks * sizeof(SiChunk)) != 0);
    if (nu > 0) two_level_differs |= memcmp(&units2[nu - 1], &units[nu - 1], sizeof(pcamv_unit_t)) != 0;      /* the last unit's entry is the prefix' */
    free(B); free(units2);
    for (long long c = 0; c < n_chunks; c++) si_scan(work, src, len, c, 1, ch + c, all);

    VgWork W = {exact<long long>(65), exact<long long>(65)};
    pcamv_gop_t *gops = exact<pcamv_gop_t>((size_t)cap);
    memset((void *)gops, 0xA5, (size_t)cap * sizeof(pcamv_gop_t));
    long long *ctx = exact<long long>(2 * (size_t)n_ctx), got_n = -7, got_pre = -7;
    for (int k = 0; k < 2 * n_ctx; k++) ctx[k] = -7;
    const VgOut O = {gops, first, cap, ctx, ctx + n_ctx, 1000, n_ctx, &got_n, &got_pre};
    vg_cut(W, units, nu, len, O);
    int differ = got_n != want_n || got_pre != want_pre || two_level_differs;
    for (long long r = 0; r < cap; r++) {
        const long long g = first + r;
        if (g < want_n) differ |= memcmp(&gops[r], &want[(size_t)g], sizeof(pcamv_gop_t)) != 0;
        else for (size_t j = 0; j < sizeof(pcamv_gop_t); j++) differ |= ((const uint8_t *)(gops + r))[j] != 0xA5;
    }
    for (int r = 0; r < n_ctx; r++) {
        const long long g = first + r;
        differ |= ctx[r] != (g < want_n ? 1000 + want[(size_t)g].off : 0) || ctx[n_ctx + r] != (g < want_n ? want[(size_t)g].len : 0);
    }
    free(work.win); free(work.sc); free(ch); free(keep); free(units); free(W.start); free(W.unit); free(gops); free(ctx);
    return differ;
}

static void check_video(const std::vector<uint8_t> &v, long long cap)
{
    const size_t len = v.size(), most = len / 4 + 1;
    std::vector<pcamv_gop_t> want(most);
    int64_t n = 0, pre = 0;
    int differ = pcamv_gpu_annexb_gops(v.data(), len, want.data(), most, &n, &pre) != 0 || (size_t)n > most;
    for (int a = 0; a < 4 && !differ; a++) {
        uint8_t *block = exact<uint8_t>(len + a);               /* ends with the video: any read past it is caught */
        memset(block, 0, a);
        if (len) memcpy(block + a, v.data(), len);
        const long long first = a & 1;
        differ |= cut_one(block + a, (long long)len, cap < 0 ? (first < n ? n - first : 0) : cap, want, n, pre, first, a & 2 ? 3 : 0);
        free(block);
    }
    n_videos++;
    if (differ) { if (n_vdiffer < 20) { printf("video differs:"); for (size_t k = 0; k < len && k < 32; k++) printf(" %02x", v[k]); printf(" (%zu bytes)\n", len); } n_vdiffer++; }
}

static uint8_t *aligned_block(size_t bytes, int a, uint8_t **base)
{
    void *p = NULL;
    if (posix_memalign(&p, 32, bytes + (size_t)a ? bytes + (size_t)a : 1)) exit(2);
    *base = (uint8_t *)p;
    return *base + a;
}

static void check_copy(int sa, int da, long long len)
{
    uint8_t *sb, *db, *src = aligned_block((size_t)len, sa, &sb), *dst = aligned_block((size_t)len, da, &db);
    std::vector<uint8_t> want((size_t)len);
    for (long long k = 0; k < len; k++) want[(size_t)k] = src[k] = (uint8_t)(k * 131 + 7 + sa);
    memset(sb, 0x3C, (size_t)sa); memset(db, 0x5A, (size_t)da + (size_t)len);
    long long *sum = exact<long long>(64), *base = exact<long long>(2);
    const VcJob job = {0, 0, len};
    vc_plan(sum, dst, &job, 1, base);
    int differ = base[0] != 0 || base[1] != vc_chunks(dst, len);
    for (long long f = 0; f < base[1]; f++) {
        long long c = -1;
        differ |= vc_job_of(base, 1, f, &c) != 0 || c != f;
        vc_copy_chunk(src, dst, len, c);
    }
    differ |= len && memcmp(dst, want.data(), (size_t)len);
    for (int k = 0; k < da; k++) differ |= db[k] != 0x5A;
    free(sb); free(db); free(sum); free(base);
    n_copies++;
    if (differ) { if (n_cdiffer < 20) printf("copy differs: source at %d, destination at %d, %lld bytes\n", sa, da, len); n_cdiffer++; }
}

/* every job in one launch: job i's source behind job i - 1's at its own alignment mod 32, the destinations likewise */
static void check_launch(const std::vector<int> &jobs)
{
    const int n = (int)jobs.size() / 3;
    std::vector<VcJob> J((size_t)n);
    long long s_at = 0, d_at = 0;
    for (int i = 0; i < n; i++) {
        s_at = (s_at + 31) / 32 * 32 + jobs[3 * i]; d_at = (d_at + 31) / 32 * 32 + jobs[3 * i + 1];
        J[(size_t)i].src = s_at; J[(size_t)i].dst = d_at; J[(size_t)i].len = jobs[3 * i + 2];
        s_at += jobs[3 * i + 2]; d_at += jobs[3 * i + 2];
    }
    uint8_t *sb, *db, *src = aligned_block((size_t)s_at, 0, &sb), *dst = aligned_block((size_t)d_at, 0, &db);
    for (long long k = 0; k < s_at; k++) src[k] = (uint8_t)(k * 29 + (k >> 8));
    memset(dst, 0x5A, (size_t)d_at);
    std::vector<uint8_t> want((size_t)d_at, 0x5A);
    for (int i = 0; i < n; i++) if (J[(size_t)i].len) memcpy(want.data() + J[(size_t)i].dst, src + J[(size_t)i].src, (size_t)J[(size_t)i].len);
    long long *sum = exact<long long>(64), *base = exact<long long>((size_t)n + 1);
    VcJob *jobs_block = exact<VcJob>((size_t)n);
    memcpy((void *)jobs_block, J.data(), (size_t)n * sizeof(VcJob));
    vc_plan(sum, dst, jobs_block, n, base);
    int differ = 0;
    long long total = 0;
    for (int i = 0; i < n; i++) { differ |= base[i] != total; total += vc_chunks(dst + J[(size_t)i].dst, J[(size_t)i].len); }
    differ |= base[n] != total;
    for (long long f = 0; f < base[n] && !differ; f++) {
        long long c = -1;
        const int i = vc_job_of(base, n, f, &c);
        differ |= i < 0 || i >= n || c < 0 || c >= vc_chunks(dst + J[(size_t)i].dst, J[(size_t)i].len) || base[i] + c != f;
        if (!differ) vc_copy_chunk(src + J[(size_t)i].src, dst + J[(size_t)i].dst, J[(size_t)i].len, c);
    }
    differ |= d_at && memcmp(dst, want.data(), (size_t)d_at);
    free(sb); free(db); free(sum); free(base); free(jobs_block);
    n_copies++;
    if (differ) { printf("the launch of all %d jobs differs\n", n); n_cdiffer++; }
}

/* 70 contexts, some refused, some empty: vj_join's jobs, placed, length and status for a video buffer with and without room */
static void check_join(long long room_short)
{
    const int n = 70;
    SwsCtx *ctx = exact<SwsCtx>(n);
    long long total = 0;
    for (int i = 0; i < n; i++) {
        const SwsCtx c = {1000LL * i + (i & 3), 900, i % 7 == 3 ? 0 : 100 + 13 * i, 0, 0, i % 11 == 5, 0};
        ctx[i] = c;
        if (!c.bad) total += c.cur;
    }
    long long *sum = exact<long long>(64), *placed = exact<long long>(n), *off = exact<long long>(1), *len = exact<long long>(1);
    int *status = exact<int>(1);
    VcJob *jobs = exact<VcJob>(n);
    *off = 3; *len = 17; *status = -7;
    const long long size = 3 + 17 + total - room_short;
    vj_join(sum, ctx, n, size, off, len, placed, status, jobs);
    const int fits = room_short <= 0;
    int differ = *status != (fits ? 0 : PCAMV_ENOMEM) || *len != (fits ? 17 + total : 17) || *off != 3;
    long long at = 17;
    for (int i = 0; i < n; i++) {
        const long long have = ctx[i].bad ? 0 : ctx[i].cur;
        differ |= placed[i] != (fits && have ? at : -1) || jobs[i].len != (fits ? have : 0);
        if (fits && have) differ |= jobs[i].src != ctx[i].off || jobs[i].dst != 3 + at;
        at += have;
    }
    free(ctx); free(sum); free(placed); free(off); free(len); free(status); free(jobs);
    n_joins++;
    if (differ) { printf("join differs (short by %lld)\n", room_short); n_jdiffer++; }
}
/* vj_head against sws_open's decision with head = the context's bytes, and the head's own refusals */
static void check_heads()
{
    const long long bytes_size = 5000, heads_size = 700;
    const long long cases[][4] = {{0, 100, 0, 50}, {1, 100, 650, 50}, {1, 100, 651, 50}, {4900, 100, 0, 100}, {4901, 100, 0, 10}, {0, 49, 0, 50}, {0, 50, 0, 50}, {7, 0, 3, 0},
                                  {7, 10, 700, 0}, {7, 10, 701, 0}, {7, 10, -1, 4}, {7, 10, 0, -1}, {-1, 10, 0, 4}, {7, -1, 0, 0}, {0, 5000, 0, 700}, {0, 5001, 0, 1}};
    for (const auto &k : cases) {
        SwsCtx c, w;
        long long len = -7, wlen = -7;
        const VcJob j = vj_head(c, bytes_size, k[0], k[1], heads_size, k[2], k[3], &len);
        const int head_in = k[3] >= 0 && k[2] >= 0 && k[3] <= heads_size && k[2] <= heads_size - k[3];
        std::vector<uint8_t> bytes((size_t)bytes_size), head((size_t)(head_in ? k[3] : 0));
        /* a head inside `heads`: stream_open's own decision with that head; else refused, the region noted as stream_open notes it */
        sws_open(w, bytes.data(), bytes_size, k[0], k[1], head.data(), head_in ? k[3] : 0, &wlen);
        if (!head_in) { w.bad = 1; w.cur = 0; wlen = 0; }
        int differ = c.bad != w.bad || c.cur != w.cur || len != wlen || c.off != w.off || c.cap != w.cap || c.pic != 0 || c.units != 0 || j.len != len;
        if (!c.bad) differ |= j.src != k[2] || j.dst != k[0];
        n_joins++;
        if (differ) { printf("head differs: off %lld cap %lld head %lld + %lld\n", k[0], k[1], k[2], k[3]); n_jdiffer++; }
    }
    SwsCtx c; long long len = -7;           /* the longest head and one byte more */
    vj_head(c, 1LL << 26, 0, 1LL << 25, 1LL << 25, 0, VC_HEAD_MAX, &len);
    int differ = c.bad || len != VC_HEAD_MAX;
    vj_head(c, 1LL << 26, 0, 1LL << 25, 1LL << 25, 0, VC_HEAD_MAX + 1, &len);
    differ |= !c.bad || len != 0;
    n_joins++;
    if (differ) { printf("head differs at the longest head\n"); n_jdiffer++; }
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t count = 0;
    if (fread(&count, 4, 1, f) != 1 || count < 0) return 2;
    for (int k = 0; k < count; k++) {
        int32_t h[2];
        if (fread(h, 4, 2, f) != 2 || h[1] < 0) return 2;
        std::vector<uint8_t> v((size_t)h[1]);
        if (h[1] && fread(v.data(), 1, v.size(), f) != v.size()) return 2;
        check_video(v, h[0]);
    }
    if (fread(&count, 4, 1, f) != 1 || count < 0) return 2;
    std::vector<int> jobs;
    for (int k = 0; k < count; k++) {
        int32_t h[3];
        if (fread(h, 4, 3, f) != 3 || h[0] < 0 || h[0] > 31 || h[1] < 0 || h[1] > 31 || h[2] < 0) return 2;
        check_copy(h[0], h[1], h[2]);
        jobs.insert(jobs.end(), h, h + 3);
    }
    fclose(f);
    check_launch(jobs);
    check_join(0); check_join(1); check_join(-5);
    check_heads();
    printf("videos %ld ok %ld differ %ld\n", n_videos, n_videos - n_vdiffer, n_vdiffer);
    printf("copies %ld ok %ld differ %ld\n", n_copies, n_copies - n_cdiffer, n_cdiffer);
    printf("joins %ld ok %ld differ %ld\n", n_joins, n_joins - n_jdiffer, n_jdiffer);
    return n_vdiffer || n_cdiffer || n_jdiffer ? 1 : 0;
}
