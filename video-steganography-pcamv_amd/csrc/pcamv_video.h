/*
 * pcamv_video.h -- one video of many chains, as control code that compiles for the device and for the host: byte ranges copied in
 * chunks (a head per context into its stream; the contexts' streams behind each other into one video), and a video cut into its GOPs.
 *
 * On the device it is the body of k_stream_open_heads, k_stream_join, k_stream_copy_plan, k_stream_copy and k_video_cut
 * (pcamv_slice.hip.h).  On the host it is what tests/fuzz/check_video.cpp compiles with the scalar form of SP_LANES
 * (pcamv_slice_parse.h), to be compared copy by copy with memcpy and video by video with pcamv_gpu_annexb_gops (pcamv_mvsyntax.h), whose
 * semantics the cut has on every input, valid or not.  No HIP type.
 *
 * The copy.  A launch has n jobs {src, dst, len}, offsets into one source and one destination buffer, made on the device by vj_head or
 * vj_join, which are what keeps them inside the buffers.  A job is cut into chunks of VC_CHUNK destination bytes at destination
 * addresses that are multiples of 16 (the first chunk is shorter by the destination's misalignment); vc_plan, one wavefront, makes the
 * exclusive prefix of the jobs' chunk counts (a lane walks its share of the jobs, the lanes' sums meet in working memory: any n), and
 * vc_job_of finds a flat chunk's job by binary search.  A wavefront takes one chunk in passes of VC_PASS bytes, 16 per lane.  A lane's
 * four destination dwords are aligned; the source is read as aligned dwords too -- a whole dword only where all four of its bytes lie
 * inside the job's source, as nu_load has it -- and funnel-shifted by the difference of the two addresses mod 4.  Where all 16 bytes
 * belong to the job they leave with one 16-byte store (a wavefront: 1 KiB per instruction), and arrive with one 16-byte load where the
 * two addresses agree mod 16; else a dword leaves whole where all four bytes belong to the job, and single bytes leave only at the two
 * ends of the job.  Nothing outside src[0, len) is read, nothing outside dst[0, len) is written.
 *
 * The cut (the rule: include/pcamv_gpu.h).  The video's units are in a table (all of them: the index kernels, pcamv_stream_index.h).
 * One wavefront walks it in passes of 64 units, a unit per lane.  Two ballots -- "is VCL", "is of type 5" -- give a lane the nearest
 * VCL unit below it, or the one carried over from the passes before; an IDR unit opens a GOP exactly if that unit is none or not of
 * type 5.  A third ballot compacts the openers: opener number g of the video writes GOP g's first byte and first unit and, knowing
 * opener g - 1's through working memory (or carried), GOP g - 1's length and unit count.  A GOP goes to the table of GOPs (the first
 * `cap` from `first` on) and, as (off, len), to context g - first; contexts past the last GOP get (0, 0).  Every entry is written by
 * one lane once.  Results leave through ordinary stores.
 */
#ifndef PCAMV_VIDEO_H
#define PCAMV_VIDEO_H
#include "pcamv_stream_write.h"

#define VC_CHUNK PCAMV_STREAM_CHUNK     /* destination bytes of a job one wavefront copies */
#define VC_PASS 1024                    /* ... in passes of 16 bytes per lane */
#define VC_HEAD_MAX (1LL << 24)         /* the longest head (pcamv_gpu_batch_stream_open's limit) */
static_assert(VC_CHUNK % VC_PASS == 0 && VC_CHUNK >= VC_PASS, "a chunk is whole passes");

struct VcJob { long long src, dst, len; };
struct Vc16 { uint32_t w[4]; };
SP_HD Vc16 vc_ld128(const void *p) { Vc16 v; __builtin_memcpy(&v, __builtin_assume_aligned(p, 16), 16); return v; }
SP_HD void vc_st128(void *p, const Vc16 &v) { __builtin_memcpy(__builtin_assume_aligned(p, 16), &v, 16); }

SP_HD long long vc_chunks(const uint8_t *dst, long long len) { return len > 0 ? (len + (long long)((uintptr_t)dst & 15u) + VC_CHUNK - 1) / VC_CHUNK : 0; }

/* one wavefront: chunk_base[0 .. n] from the jobs' chunk counts, chunk_base[n] their sum.  sum: 64 entries of working memory */
SP_HD void vc_plan(long long *sum, const uint8_t *dst, const VcJob *jobs, int n, long long *chunk_base)
{
    const int seg = (n + 63) / 64;
    SP_SYNC();
    SP_LANES(l) {
        long long s = 0;
        for (int i = l * seg; i < (l + 1) * seg && i < n; i++) s += vc_chunks(dst + jobs[i].dst, jobs[i].len);
        sum[l] = s;
    }
    SP_SYNC();
    SP_LANES(l) {
        long long base = 0;
        for (int j = 0; j < l; j++) base += sum[j];
        for (int i = l * seg; i < (l + 1) * seg && i < n; i++) {
            chunk_base[i] = base;
            base += vc_chunks(dst + jobs[i].dst, jobs[i].len);
            if (i == n - 1) chunk_base[n] = base;
        }
        if (n == 0 && l == 0) chunk_base[0] = 0;
    }
}
/* the job flat chunk f < chunk_base[n] belongs to -- jobs without chunks share their base with the job behind them, so it is the last
 * one whose base is not above f -- and the chunk's number there */
SP_HD int vc_job_of(const long long *chunk_base, int n, long long f, long long *c)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (chunk_base[mid] <= f) lo = mid; else hi = mid - 1; }
    *c = f - chunk_base[lo];
    return lo;
}
/* chunk c of the job src[0, len) -> dst[0, len) */
SP_HD void vc_copy_chunk(const uint8_t *src, uint8_t *dst, long long len, long long c)
{
    const long long lo = c * VC_CHUNK - (long long)((uintptr_t)dst & 15u), hi = lo + VC_CHUNK < len ? lo + VC_CHUNK : len;   /* lo < 0 in chunk 0 of a misaligned job */
    const int s = (int)(((uintptr_t)src - (uintptr_t)dst) & 3u), s16 = (int)(((uintptr_t)src - (uintptr_t)dst) & 15u);
    for (long long pb = lo; pb < hi; pb += VC_PASS) {
        SP_LANES(l) {
            const long long p = pb + 16 * l;            /* dst + p is a multiple of 16, src + p - s one of 4 */
            if (p >= hi || p + 16 <= 0) continue;
            const int whole = p >= 0 && p + 16 <= len;
            Vc16 o;
            if (whole && s16 == 0) o = vc_ld128(src + p);
            else {
                uint32_t w[5];
                for (int k = 0; k < 5; k++) w[k] = k < 4 || s ? nu_load(src, len, p - s + 4 * k) : 0u;
                for (int k = 0; k < 4; k++) o.w[k] = s ? w[k] >> (8 * s) | w[k + 1] << (32 - 8 * s) : w[k];
            }
            if (whole) { vc_st128(dst + p, o); continue; }
            for (int k = 0; k < 4; k++) {
                const long long q = p + 4 * k;
                if (q >= 0 && q + 4 <= len) sp_st32(dst + q, o.w[k]);
                else for (int j = 0; j < 4; j++) if (q + j >= 0 && q + j < len) dst[q + j] = (uint8_t)(o.w[k] >> (8 * j));
            }
        }
    }
}

/* ---- the jobs.  Context i of an open with a head per context: sws_open's decision with the head's own place judged too; the job that
 * copies the head, of length 0 for a context that is refused */
SP_HD VcJob vj_head(SwsCtx &c, long long bytes_size, long long off, long long cap, long long heads_size, long long head_off, long long head_len, long long *len)
{
    c.off = off; c.cap = cap; c.cur = 0; c.pic = 0; c.units = 0; c.pad = 0;
    const int head_in = head_len >= 0 && head_len <= VC_HEAD_MAX && head_off >= 0 && head_len <= heads_size && head_off <= heads_size - head_len;
    c.bad = !(off >= 0 && cap >= 0 && cap <= bytes_size && off <= bytes_size - cap && head_in && head_len <= cap);
    if (!c.bad) c.cur = head_len;
    *len = c.cur;
    const VcJob j = {c.bad ? 0 : head_off, c.bad ? 0 : off, c.cur};
    return j;
}
/* one wavefront: the streams of contexts 0 .. n - 1 behind video[*video_off + *video_len ..), if they fit video_size (else no job has a
 * length, *video_len stays and *status is PCAMV_ENOMEM).  A lane walks its share of the contexts.  sum: 64 entries of working memory */
SP_HD void vj_join(long long *sum, const SwsCtx *ctx, int n, long long video_size, const long long *video_off, long long *video_len, long long *placed,
                   int *status, VcJob *jobs)
{
    const int seg = (n + 63) / 64;
    const long long v_off = *video_off, v_len = *video_len;
    SP_SYNC();
    SP_LANES(l) {
        long long s = 0;
        for (int i = l * seg; i < (l + 1) * seg && i < n; i++) if (!ctx[i].bad && ctx[i].cur > 0) s += ctx[i].cur;
        sum[l] = s;
    }
    SP_SYNC();
    long long total = 0;
    for (int j = 0; j < 64; j++) total += sum[j];
    const int fits = v_off >= 0 && v_len >= 0 && v_off <= video_size && v_len <= video_size - v_off && total <= video_size - v_off - v_len;
    SP_LANES(l) {
        long long at = v_len;
        for (int j = 0; j < l; j++) at += sum[j];
        for (int i = l * seg; i < (l + 1) * seg && i < n; i++) {
            const long long have = !ctx[i].bad && ctx[i].cur > 0 ? ctx[i].cur : 0;
            const VcJob j = {have && fits ? ctx[i].off : 0, have && fits ? v_off + at : 0, fits ? have : 0};
            jobs[i] = j;
            if (placed) placed[i] = have && fits ? at : -1;
            at += have;
        }
    }
    SP_SYNC();
    SP_LANES(l) if (l == 0) { if (fits) *video_len = v_len + total; *status = fits ? 0 : PCAMV_ENOMEM; }
}

/* ---- the index of ONE long stream.  si_prefix is one wavefront per stream, serial over the stream's chunks in passes of 64: right for
 * thousands of streams of a few chunks, and 15 ms for a video of 4096 CIF chains as one stream of 174 k chunks.  Sums and maxima are
 * associative, so the same prefix in two levels: vp_local, a wavefront per block of VP_BLOCK chunks, is si_prefix on the block alone
 * (its exclusive prefix in place, its totals to B[block]); si_prefix itself then runs over B, where it also makes the stream's totals
 * and its last unit's entry as it always does; vp_apply, a lane per chunk, puts the block's base under the chunk's local prefix */
#define VP_BLOCK 64
SP_HD void vp_local(const SiWork &W, const uint8_t *src, long long len, SiChunk *ch, long long n_chunks, long long blk, SiChunk *B)
{
    const long long left = n_chunks - blk * VP_BLOCK, cnt = left < VP_BLOCK ? left : VP_BLOCK;
    const SiTable none = {NULL, 0, 1, NULL, 0};
    si_prefix(W, src, len, ch + blk * VP_BLOCK, cnt, none, &B[blk].units, &B[blk].slices);
    SP_SYNC();
    SP_LANES(l) if (l == 0) {           /* (W.sc still holds the block's summaries, "none" behind the last) */
        long long nz = -1, q = -1;
        for (int j = 0; j < 64; j++) { if (W.sc[j].nz > nz) nz = W.sc[j].nz; if (W.sc[j].q > q) q = W.sc[j].q; }
        B[blk].nz = nz; B[blk].q = q;
    }
}
SP_HD void vp_apply(SiChunk *ch, long long n_chunks, const SiChunk *B, long long i)
{
    if (i >= n_chunks) return;
    const SiChunk b = B[i / VP_BLOCK];
    SiChunk c = ch[i];
    c.units += b.units; c.slices += b.slices;
    if (b.nz > c.nz) c.nz = b.nz;
    if (b.q > c.q) c.q = b.q;
    ch[i] = c;
}

/* ---- the cut */
struct VgWork { long long *start, *unit; };     /* 65 entries each: [0] the opener before the pass, [1 ..] the pass' openers in order */
/* where the GOPs go: gops[0, cap) takes GOPs first .. first + cap - 1, contexts 0 .. n_ctx - 1 take GOPs first .. as (base + off, len) */
struct VgOut { pcamv_gop_t *gops; long long first, cap; long long *ctx_off, *ctx_len; long long base; int n_ctx; long long *n_gops, *preamble; };
SP_HD void vg_begin(const VgOut &O, long long g, long long at, long long unit)
{
    const long long r = g - O.first;
    if (r < 0) return;
    if (r < O.cap) { O.gops[r].off = at; O.gops[r].first_unit = unit; }
    if (r < O.n_ctx) O.ctx_off[r] = O.base + at;
}
SP_HD void vg_end(const VgOut &O, long long g, long long at, long long unit, long long next_at, long long next_unit)
{
    const long long r = g - O.first;
    if (r < 0) return;
    if (r < O.cap) { O.gops[r].len = next_at - at; O.gops[r].n_units = next_unit - unit; }
    if (r < O.n_ctx) O.ctx_len[r] = next_at - at;
}
/* one wavefront: the video of `len` bytes whose m units are U[0, m) */
SP_HD void vg_cut(const VgWork &W, const pcamv_unit_t *U, long long m, long long len, const VgOut &O)
{
    long long n_gops = 0, last_vcl = -1, prev_at = 0, prev_unit = 0, first_at = len;
    int last5 = 0;
    for (long long g = 0; g < m; g += 64) {
        uint64_t mv = 0, m5 = 0, mo = 0;
        long long at[SP_SLOTS], unit[SP_SLOTS];
        SP_SYNC();
        SP_LANES(l) {
            const int h = g + l < m ? U[g + l].nal_header : -1, t = h < 0 ? 0 : h & 31;
            NU_VOTE(mv, l, t >= 1 && t <= 5); NU_VOTE(m5, l, t == 5);
        }
        SP_LANES(l) {
            const uint64_t below = mv & (((uint64_t)1 << l) - 1u);
            long long pv = last_vcl;
            int p5 = last5;
            if (below) { const int j = si_top(below); pv = g + j; p5 = (int)((m5 >> j) & 1u); }
            const int opens = (int)((m5 >> l) & 1u) && !(pv >= 0 && p5);
            const long long f = pv + 1;
            long long a = 0;
            if (opens && f > 0) a = U[f - 1].off + U[f - 1].len;
            at[SP_SLOT(l)] = a; unit[SP_SLOT(l)] = f;
            NU_VOTE(mo, l, opens);
        }
        SP_LANES(l) {
            if ((mo >> l) & 1u) { const int k = nu_below(mo, l); W.start[k + 1] = at[SP_SLOT(l)]; W.unit[k + 1] = unit[SP_SLOT(l)]; }
            if (l == 0) { W.start[0] = prev_at; W.unit[0] = prev_unit; }
        }
        SP_SYNC();
        SP_LANES(l) {
            if (!((mo >> l) & 1u)) continue;
            const int k = nu_below(mo, l);
            vg_begin(O, n_gops + k, at[SP_SLOT(l)], unit[SP_SLOT(l)]);
            if (n_gops + k > 0) vg_end(O, n_gops + k - 1, W.start[k], W.unit[k], at[SP_SLOT(l)], unit[SP_SLOT(l)]);
        }
        const int openers = __builtin_popcountll(mo);
        if (openers) {
            if (n_gops == 0) first_at = W.start[1];
            prev_at = W.start[openers]; prev_unit = W.unit[openers];
            n_gops += openers;
        }
        if (mv) { const int j = si_top(mv); last_vcl = g + j; last5 = (int)((m5 >> j) & 1u); }
    }
    SP_LANES(l) {
        if (l == 0) {
            if (n_gops > 0) vg_end(O, n_gops - 1, prev_at, prev_unit, len, m);
            *O.n_gops = n_gops; *O.preamble = first_at;
        }
        for (long long r = l; r < O.n_ctx; r += 64) if (r >= n_gops - O.first) { O.ctx_off[r] = 0; O.ctx_len[r] = 0; }
    }
}
#endif
