/*
 * pcamv_idr.hip -- the IDR picture of every chain coded on the device (gfx950): k_idr_mb, k_idr_mb4, k_idr_prefix, k_idr_pack, k_idr_slot,
 * k_idr_unit, k_idr_deblock.  The coder itself is pcamv_idr.h with pcamv_idr_i4x4.h, its loop filter pcamv_idr_deblock.h (all shared with the host checks);
 * this unit gives them their working memory and their place in a batch.
 *
 *   k_idr_mb      one wavefront per macroblock, launched once per anti-diagonal x + y = d over the contexts of a group (Intra16x16 reads
 *                 left, top and top-left only): mode decision, transform, reconstruction, counts, the macroblock's bit string.  The
 *                 working memory is LDS of the wave (IdrWork); the code tables are read where they lie.
 *   k_idr_mb4     in k_idr_mb's place in a call with i4x4 != 0 (IdrJobs::i4x4): the same macroblock, then the Intra4x4 trial -- sixteen
 *                 blocks one after the other, a wave barrier between them, a lane per candidate mode, the winner's lane coding the block --
 *                 the decision and, where Intra4x4 wins, its luma, counts, modes and bit string (idr_mb4; IdrWork and IdrWork4, 6080 bytes of
 *                 LDS).  Launched once per anti-diagonal x + 2 y = d: Intra4x4 reads the macroblock above-right.
 *   k_idr_prefix  per context the exclusive prefix of the macroblocks' bit counts, the header's bits in front: every thread sums a run
 *                 of macroblocks, the block scans the runs' sums in LDS, every thread writes its run.
 *   k_idr_pack    one lane per destination dword of the RBSP (idr_pack_dword).
 *   k_idr_slot    (streams) one lane per context: the access unit delimiter 09 10 at the stream's end, the place the unit gets.
 *   k_idr_unit    one wavefront per context: start code, header byte and emulation prevention through the slice writers' output path,
 *                 nothing stored at or beyond the capacity.
 *   k_idr_deblock one wavefront per macroblock, launched once per anti-diagonal x + 2 y = d over ALL contexts of the call, behind the
 *                 groups: it works on the contexts' reconstruction planes alone (idr_deblock_mb), in 688 bytes of LDS.
 * A picture of S > 1 slices (IdrJobs::n_slices; whole macroblock rows, the layout in pcamv_idr_defs.h) goes through k_idr_mb with availability
 * by slice, then k_idr_prefix_slices, k_idr_pack_slices, k_idr_unit_len (one wavefront per (context, slice): the unit's length by the
 * writer's own walk, stores suppressed), k_idr_place (one lane per context: the units' places, all or none) and k_idr_unit_slices (one
 * wavefront per (context, slice) into exactly its own bytes).  A picture of one slice is launched as it always was.
 * No spin-wait and no dependency between the waves of a launch.  Every store is an ordinary vector store.  Nothing else is defined here.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pcamv_flow.hip.h"
#include "pcamv_idr_i4x4.h"
#include "pcamv_idr_deblock.h"

/* context i's picture at its place in the group */
static __device__ IdrPic idr_pic(const IdrJobs &J, int i, int place)
{
    const FrameDev &F = J.Fs[i];
    const int off = F.chroma_qp_offset < -12 ? -12 : F.chroma_qp_offset > 12 ? 12 : F.chroma_qp_offset;
    IdrPic P;
    for (int k = 0; k < 3; k++) { P.src[k] = F.fenc[k]; P.rec[k] = F.rec[k]; }
    P.mb_w = F.mb_w; P.mb_h = J.n_mb / F.mb_w; P.qp = J.qp; P.qpc = J.qpc_of[12 + off]; P.dz = J.dz;
    P.nz = J.nz + (size_t)place * IDR_NZ_BYTES * J.n_mb; P.slots = J.slots + (size_t)place * IDR_SLOT_DWORDS * J.n_mb; P.bits = J.bits + (size_t)place * J.n_mb;
    P.clamped = nullptr;
    P.slice_rows = J.slice_rows;
    return P;
}

static __global__ void __launch_bounds__(64) k_idr_mb(const IdrJobs J, int d, int g0)
{
    __shared__ IdrWork W;
    const IdrPic P = idr_pic(J, g0 + blockIdx.y, blockIdx.y);
    const int y_lo = d - (P.mb_w - 1) > 0 ? d - (P.mb_w - 1) : 0, my = y_lo + (int)blockIdx.x, mx = d - my;
    if (my >= P.mb_h || mx < 0 || mx >= P.mb_w) return;
    idr_mb(W, P, (const uint16_t *)J.tab, mx, my);
}

/* a call with i4x4 != 0: the same macroblock and then the Intra4x4 trial, the decision and, where it wins, the Intra4x4 macroblock
 * (idr_mb4).  Intra4x4 reads the macroblock above-right, which x + y does not order: one launch per anti-diagonal x + 2 y = d */
static __global__ void __launch_bounds__(64) k_idr_mb4(const IdrJobs J, int d, int g0)
{
    __shared__ IdrWork W;
    __shared__ IdrWork4 W4;
    IdrPic P = idr_pic(J, g0 + blockIdx.y, blockIdx.y);
    if (!J.modes) return;
    P.i4x4 = J.i4x4; P.lambda = J.lambda; P.modes = J.modes + (size_t)blockIdx.y * IDR_MODE_BYTES * J.n_mb;      /* (this kernel's alone: the others leave them at their defaults) */
    int y_lo, y_hi;
    idb_diag_rows(d, P.mb_w, P.mb_h, &y_lo, &y_hi);
    const int my = y_lo + (int)blockIdx.x, mx = d - 2 * my;
    if (my > y_hi || mx < 0 || mx >= P.mb_w) return;
    idr_mb4(W, W4, P, (const uint16_t *)J.tab, mx, my);
}

#define IDR_PREFIX_THREADS 1024
static __global__ void __launch_bounds__(IDR_PREFIX_THREADS) k_idr_prefix(const IdrJobs J, int g0)
{
    __shared__ long long s_sum[IDR_PREFIX_THREADS];
    __shared__ int s_bad;
    const int i = g0 + blockIdx.x, t = threadIdx.x;
    const IdrPic P = idr_pic(J, i, blockIdx.x);
    const int n_mb = P.mb_w * P.mb_h, run = (n_mb + IDR_PREFIX_THREADS - 1) / IDR_PREFIX_THREADS;
    const int lo = t * run < n_mb ? t * run : n_mb, hi = lo + run < n_mb ? lo + run : n_mb;
    long long *pre = J.pre + (long long)blockIdx.x * (J.n_mb + 1);
    if (t == 0) s_bad = 0;
    __syncthreads();
    long long sum = 0;
    int bad = 0;
    for (int k = lo; k < hi; k++) { const int b = P.bits[k]; if (b < 0) bad = 1; else sum += b; }
    if (bad) s_bad = 1;
    s_sum[t] = sum;
    __syncthreads();
    for (int step = 1; step < IDR_PREFIX_THREADS; step <<= 1) {
        const long long v = t >= step ? s_sum[t - step] : 0;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    long long at = J.hdr_bits + s_sum[t] - sum;
    for (int k = lo; k < hi; k++) { pre[k] = at; const int b = P.bits[k]; at += b < 0 ? 0 : b; }
    if (t == IDR_PREFIX_THREADS - 1) { pre[n_mb] = J.hdr_bits + s_sum[t]; J.bad[i] = s_bad; }
}

static __global__ void __launch_bounds__(256) k_idr_pack(const IdrJobs J, int g0)
{
    const IdrPic P = idr_pic(J, g0 + blockIdx.y, blockIdx.y);
    const int n_mb = P.mb_w * P.mb_h;
    const long long *pre = J.pre + (long long)blockIdx.y * (J.n_mb + 1);
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x, dwords = (idr_rbsp_bytes(pre[n_mb]) + 3) >> 2;
    if (k >= dwords || k >= J.rbsp_stride / 4) return;
    ((uint32_t *)(J.rbsp + (long long)blockIdx.y * J.rbsp_stride))[k] = idr_pack_dword(k, J.hdr, J.hdr_bits, pre, P.slots, n_mb);
}

/* ---- several slices per picture (J.n_slices = S > 1; the layout: pcamv_idr_defs.h).  A place's prefix array has J.n_mb + S entries.
 * The prefix restarts at every slice behind that slice's header: the block's scan gives every macroblock the bits of all before it in
 * the picture, written first where the macroblock's entry lies; every slice then takes the value at its first macroblock (kept in the
 * place's uoff, which k_idr_place fills only later) and writes its stop bit's entry, which is no macroblock's; then every thread turns
 * its own entries into the slice's.  A thread's run may hold a slice boundary: the slice is found per macroblock. */
static __global__ void __launch_bounds__(IDR_PREFIX_THREADS) k_idr_prefix_slices(const IdrJobs J, int g0)
{
    __shared__ long long s_sum[IDR_PREFIX_THREADS];
    __shared__ int s_bad;
    const int i = g0 + blockIdx.x, t = threadIdx.x, S = J.n_slices;
    const IdrPic P = idr_pic(J, i, blockIdx.x);
    const int n_mb = P.mb_w * P.mb_h, run = (n_mb + IDR_PREFIX_THREADS - 1) / IDR_PREFIX_THREADS;
    const int lo = t * run < n_mb ? t * run : n_mb, hi = lo + run < n_mb ? lo + run : n_mb;
    long long *pre = J.pre + (long long)blockIdx.x * (J.n_mb + S), *base = J.uoff + (long long)blockIdx.x * S;
    if (t == 0) s_bad = 0;
    __syncthreads();
    long long sum = 0;
    int bad = 0;
    for (int k = lo; k < hi; k++) { const int b = P.bits[k]; if (b < 0) bad = 1; else sum += b; }
    if (bad) s_bad = 1;
    s_sum[t] = sum;
    __syncthreads();
    for (int step = 1; step < IDR_PREFIX_THREADS; step <<= 1) {
        const long long v = t >= step ? s_sum[t - step] : 0;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    const long long total = s_sum[IDR_PREFIX_THREADS - 1];
    long long at = s_sum[t] - sum;
    for (int k = lo; k < hi; k++) {
        pre[k + idr_slice_of_row(P.mb_h, P.slice_rows, k / P.mb_w)] = at;
        const int b = P.bits[k]; at += b < 0 ? 0 : b;
    }
    __syncthreads();
    for (int s = t; s < S; s += IDR_PREFIX_THREADS) {
        const long long f = idr_slice_first_mb(P.mb_w, P.mb_h, P.slice_rows, s), n = idr_slice_n_mb(P.mb_w, P.mb_h, P.slice_rows, s);
        const long long first = pre[idr_slice_pre_at(f, s)], next = s + 1 < S ? pre[idr_slice_pre_at(f + n, s + 1)] : total;
        base[s] = first;
        pre[idr_slice_pre_at(f, s) + n] = J.shdr[s].bits + next - first;
    }
    __syncthreads();
    for (int k = lo; k < hi; k++) {
        const int s = idr_slice_of_row(P.mb_h, P.slice_rows, k / P.mb_w);
        pre[k + s] += J.shdr[s].bits - base[s];
    }
    if (t == 0) J.bad[i] = s_bad;
}

/* blockIdx.y + q0 = place * S + slice; one lane per destination dword of that slice's RBSP */
static __global__ void __launch_bounds__(256) k_idr_pack_slices(const IdrJobs J, int g0, int q0)
{
    const int S = J.n_slices, q = q0 + (int)blockIdx.y, place = q / S, s = q - place * S;
    const IdrPic P = idr_pic(J, g0 + place, place);
    const long long f = idr_slice_first_mb(P.mb_w, P.mb_h, P.slice_rows, s), n = idr_slice_n_mb(P.mb_w, P.mb_h, P.slice_rows, s);
    const long long *pre = J.pre + (long long)place * (J.n_mb + S) + idr_slice_pre_at(f, s);
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x, dwords = (idr_rbsp_bytes(pre[n]) + 3) >> 2;
    const long long at = idr_slice_rbsp_at_bits(f, s, J.mb_bits), room = (idr_slice_rbsp_at_bits(f + n, s + 1, J.mb_bits) - at) / 4;
    if (k >= dwords || k >= room) return;
    ((uint32_t *)(J.rbsp + (long long)place * J.rbsp_stride + at))[k] = idr_pack_dword(k, J.shdr[s].hdr, J.shdr[s].bits, pre, P.slots + (size_t)f * IDR_SLOT_DWORDS, (int)n);
}

/* one wavefront per (place, slice): the length its unit will have, by the writer's own walk with every store suppressed */
static __global__ void __launch_bounds__(64) k_idr_unit_len(const IdrJobs J, int g0)
{
    __shared__ uint32_t s_win[64], s_obuf[SW_OBUF / 4];
    const int S = J.n_slices, place = (int)(blockIdx.x / (unsigned)S), s = (int)blockIdx.x - place * S, i = g0 + place;
    const IdrPic P = idr_pic(J, i, place);
    const long long f = idr_slice_first_mb(P.mb_w, P.mb_h, P.slice_rows, s), n = idr_slice_n_mb(P.mb_w, P.mb_h, P.slice_rows, s);
    const long long *pre = J.pre + (long long)place * (J.n_mb + S) + idr_slice_pre_at(f, s);
    const long long at = idr_slice_rbsp_at_bits(f, s, J.mb_bits), rbsp_len = idr_rbsp_bytes(pre[n]);
    long long len = -1;
    IdrOut O;
    O.obuf = s_obuf;
    if (!J.bad[i] && rbsp_len >= 0 && at + ((rbsp_len + 3) & ~3LL) <= idr_slice_rbsp_at_bits(f + n, s + 1, J.mb_bits))
        idr_unit_walk(O, s_win, J.rbsp + (long long)place * J.rbsp_stride + at, rbsp_len, J.nal_byte, J.as_nal, J.bytes, 0, 1, &len);
    if (threadIdx.x == 0) J.ulen[(long long)place * S + s] = len;
}

/* one lane per context: where its S units go, or that they do not fit -- all of them or none */
static __global__ void __launch_bounds__(64) k_idr_place(const IdrJobs J, int g0, int g)
{
    const int place = blockIdx.x * 64 + threadIdx.x, i = g0 + place, S = J.n_slices;
    if (place >= g) return;
    const long long off = J.off[i], cap = J.cap[i];
    long long total = 0;
    int rc = PCAMV_EINVAL;
    if (off >= 0 && cap >= 0 && cap <= J.bytes_size && off <= J.bytes_size - cap && !J.bad[i])
        rc = idr_place(J.ulen + (long long)place * S, J.uoff + (long long)place * S, S, cap, &total);
    J.status[i] = rc; J.len[i] = rc ? 0 : total;
    if (!rc && J.units) J.units[i].units += S - 1;      /* (k_stream_commit behind this call counts one unit for a picture that is there) */
}

/* one wavefront per (place, slice), writing at the place k_idr_place gave it, into exactly the bytes k_idr_unit_len counted: units that
 * are neighbours share a dword, and sw_flush stores the bytes of a dword that is not wholly inside [dst, dst + cap) one by one */
static __global__ void __launch_bounds__(64) k_idr_unit_slices(const IdrJobs J, int g0)
{
    __shared__ uint32_t s_win[64], s_obuf[SW_OBUF / 4];
    const int S = J.n_slices, place = (int)(blockIdx.x / (unsigned)S), s = (int)blockIdx.x - place * S, i = g0 + place;
    if (J.status[i]) return;
    const IdrPic P = idr_pic(J, i, place);
    const long long f = idr_slice_first_mb(P.mb_w, P.mb_h, P.slice_rows, s), n = idr_slice_n_mb(P.mb_w, P.mb_h, P.slice_rows, s);
    const long long *pre = J.pre + (long long)place * (J.n_mb + S) + idr_slice_pre_at(f, s);
    const long long at = idr_slice_rbsp_at_bits(f, s, J.mb_bits), rbsp_len = idr_rbsp_bytes(pre[n]);
    const long long uoff = J.uoff[(long long)place * S + s], ulen = J.ulen[(long long)place * S + s];
    long long len = 0;
    IdrOut O;
    O.obuf = s_obuf;
    if (uoff < 0 || ulen < 0 || uoff > J.cap[i] - ulen) return;         /* (k_idr_place's sum is within the capacity, which it judged) */
    idr_unit(O, s_win, J.rbsp + (long long)place * J.rbsp_stride + at, rbsp_len, J.nal_byte, J.as_nal, J.bytes + J.off[i] + uoff, ulen, &len);
}

/* the sibling of k_stream_slot for a picture whose unit is made here: the delimiter and the unit succeed or fail together */
static __global__ void __launch_bounds__(64) k_idr_slot(const IdrJobs J, const SwsCtx *ctx, int n)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const SwsCtx c = ctx[i];
    long long off = 0, cap = -1; int first = PCAMV_EINVAL;
    if (!c.bad) {
        const long long aud = J.aud ? IDR_AUD_BYTES : 0, room = c.cap - c.cur;
        off = c.off + c.cur; cap = 0; first = PCAMV_ENOMEM;
        if (room >= aud) {
            if (aud) { uint8_t *p = J.bytes + off; p[0] = 0; p[1] = 0; p[2] = 0; p[3] = 1; p[4] = 0x09; p[5] = 0x10; }      /* primary_pic_type 0 (I), the stop bit */
            off += aud; cap = room - aud; first = 0;
        }
    }
    J.off[i] = off; J.cap[i] = cap; J.first[i] = first;
}

static __global__ void __launch_bounds__(64) k_idr_unit(const IdrJobs J, int g0)
{
    __shared__ uint32_t s_win[64], s_obuf[SW_OBUF / 4];
    const int i = g0 + blockIdx.x;
    const IdrPic P = idr_pic(J, i, blockIdx.x);
    const long long *pre = J.pre + (long long)blockIdx.x * (J.n_mb + 1);
    const long long off = J.off[i], cap = J.cap[i], rbsp_len = idr_rbsp_bytes(pre[P.mb_w * P.mb_h]);
    long long len = 0;
    int rc = PCAMV_EINVAL;
    IdrOut O;
    O.obuf = s_obuf;
    if (off >= 0 && cap >= 0 && cap <= J.bytes_size && off <= J.bytes_size - cap && !J.bad[i] && rbsp_len <= J.rbsp_stride)
        rc = idr_unit(O, s_win, J.rbsp + (long long)blockIdx.x * J.rbsp_stride, rbsp_len, J.nal_byte, J.as_nal, J.bytes + off, cap, &len);
    if (threadIdx.x == 0) { J.status[i] = rc; J.len[i] = rc ? 0 : len; }
}

/* the whole picture is coded: the loop filter of an all-Intra16x16 picture at one QP needs nothing but the planes */
static __global__ void __launch_bounds__(64) k_idr_deblock(const IdrJobs J, int d, int i0)
{
    __shared__ IdbWork W;
    const FrameDev &F = J.Fs[i0 + blockIdx.y];
    const int off = F.chroma_qp_offset < -12 ? -12 : F.chroma_qp_offset > 12 ? 12 : F.chroma_qp_offset;
    IdbPic P;
    for (int k = 0; k < 3; k++) P.rec[k] = F.rec[k];
    P.mb_w = F.mb_w; P.mb_h = J.n_mb / F.mb_w; P.qp = J.qp; P.qpc = J.qpc_of[12 + off];
    int y_lo, y_hi;
    idb_diag_rows(d, P.mb_w, P.mb_h, &y_lo, &y_hi);
    const int my = y_lo + (int)blockIdx.x, mx = d - 2 * my;
    if (my > y_hi || mx < 0 || mx >= P.mb_w || P.qp < 0 || P.qp > 51) return;
    idr_deblock_mb(W, P, mx, my);
}

void pcamv_launch_idr_mb(const IdrJobs &J, int g0, int g, int mb_w, int mb_h, hipStream_t st)
{
    for (int d = 0; d < mb_w + mb_h - 1; d++) {
        const int y_lo = d - (mb_w - 1) > 0 ? d - (mb_w - 1) : 0, y_hi = d < mb_h - 1 ? d : mb_h - 1;
        hipLaunchKernelGGL(k_idr_mb, dim3((unsigned)(y_hi - y_lo + 1), (unsigned)g), dim3(64), 0, st, J, d, g0);
    }
}
void pcamv_launch_idr_mb4(const IdrJobs &J, int g0, int g, int mb_w, int mb_h, hipStream_t st)
{
    for (int d = 0; d < idb_n_diag(mb_w, mb_h); d++) {
        int y_lo, y_hi;
        idb_diag_rows(d, mb_w, mb_h, &y_lo, &y_hi);
        if (y_hi < y_lo) continue;                      /* a picture one macroblock wide has nothing on its odd diagonals */
        hipLaunchKernelGGL(k_idr_mb4, dim3((unsigned)(y_hi - y_lo + 1), (unsigned)g), dim3(64), 0, st, J, d, g0);
    }
}
int pcamv_idr_deblock_launches(int mb_w, int mb_h) { return idb_n_diag(mb_w, mb_h); }
void pcamv_launch_idr_deblock(const IdrJobs &J, int n, int mb_w, int mb_h, hipStream_t st)
{
    for (int d = 0; d < idb_n_diag(mb_w, mb_h); d++) {
        int y_lo, y_hi;
        idb_diag_rows(d, mb_w, mb_h, &y_lo, &y_hi);
        if (y_hi < y_lo) continue;                      /* a picture one macroblock wide has nothing on its odd diagonals */
        for (int i0 = 0; i0 < n; i0 += 65535)           /* (a grid's second dimension) */
            hipLaunchKernelGGL(k_idr_deblock, dim3((unsigned)(y_hi - y_lo + 1), (unsigned)(n - i0 < 65535 ? n - i0 : 65535)), dim3(64), 0, st, J, d, i0);
    }
}
void pcamv_launch_idr_prefix(const IdrJobs &J, int g0, int g, hipStream_t st) { hipLaunchKernelGGL(k_idr_prefix, dim3((unsigned)g), dim3(IDR_PREFIX_THREADS), 0, st, J, g0); }
void pcamv_launch_idr_pack(const IdrJobs &J, int g0, int g, hipStream_t st)
{
    const long long dwords = J.rbsp_stride / 4;
    hipLaunchKernelGGL(k_idr_pack, dim3((unsigned)((dwords + 255) / 256), (unsigned)g), dim3(256), 0, st, J, g0);
}
void pcamv_launch_idr_unit(const IdrJobs &J, int g0, int g, hipStream_t st) { hipLaunchKernelGGL(k_idr_unit, dim3((unsigned)g), dim3(64), 0, st, J, g0); }
/* the same four stages of a picture of several slices (J.n_slices > 1) */
void pcamv_launch_idr_prefix_slices(const IdrJobs &J, int g0, int g, hipStream_t st) { hipLaunchKernelGGL(k_idr_prefix_slices, dim3((unsigned)g), dim3(IDR_PREFIX_THREADS), 0, st, J, g0); }
void pcamv_launch_idr_pack_slices(const IdrJobs &J, int g0, int g, int mb_w, int mb_h, hipStream_t st)
{
    /* the longest slice is the first; its room in dwords bounds every slice's */
    const long long dwords = idr_slice_rbsp_at_bits(idr_slice_n_mb(mb_w, mb_h, J.slice_rows, 0), 1, J.mb_bits) / 4, total = (long long)g * J.n_slices;
    for (long long q0 = 0; q0 < total; q0 += 65535)     /* (a grid's second dimension) */
        hipLaunchKernelGGL(k_idr_pack_slices, dim3((unsigned)((dwords + 255) / 256), (unsigned)(total - q0 < 65535 ? total - q0 : 65535)), dim3(256), 0, st, J, g0, (int)q0);
}
void pcamv_launch_idr_unit_len(const IdrJobs &J, int g0, int g, hipStream_t st) { hipLaunchKernelGGL(k_idr_unit_len, dim3((unsigned)g * (unsigned)J.n_slices), dim3(64), 0, st, J, g0); }
void pcamv_launch_idr_place(const IdrJobs &J, int g0, int g, hipStream_t st) { hipLaunchKernelGGL(k_idr_place, dim3((unsigned)((g + 63) / 64)), dim3(64), 0, st, J, g0, g); }
void pcamv_launch_idr_unit_slices(const IdrJobs &J, int g0, int g, hipStream_t st) { hipLaunchKernelGGL(k_idr_unit_slices, dim3((unsigned)g * (unsigned)J.n_slices), dim3(64), 0, st, J, g0); }
void pcamv_launch_idr_slot(const IdrJobs &J, const void *sws_ctx, int n, hipStream_t st)
{
    hipLaunchKernelGGL(k_idr_slot, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, J, (const SwsCtx *)sws_ctx, n);
}
