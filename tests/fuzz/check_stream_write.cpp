/* The control code of the sender's byte streams (csrc/pcamv_stream_write.h: k_stream_open, k_stream_slot, k_stream_commit,
 * k_slice_headers_write, and the host function pcamv_gpu_write_slice_header) under AddressSanitizer + UBSan on the CPU, against a case
 * file that tests/stream_write_cases.py makes with the tests' own header writer and a naive restatement of a stream's rules.
 *
 * Headers: every case's bits are counted first (no destination), then written into a heap block of exactly (n_bits + 7) / 8 bytes -- a
 * byte more would be caught -- and compared with the file's; a refused case must give the file's code and 0 bits.
 * Sequences: the caller's buffer is a heap block of exactly bytes_size bytes filled with 0xA5 (a region the open must refuse may lie
 * anywhere: nothing of it may be touched), the header table an exact-size block for n contexts of which context i is the one that runs
 * (the other entries and slots must keep their pattern).  The slice writer is a stand-in: given the slot's (off, cap) it refuses
 * cap < 0 with PCAMV_EINVAL, writes a unit of the scripted length as bytes 0x40 + step if it fits, else stores what fits below cap and
 * fails with PCAMV_ENOMEM, as the real writers may.  After every step the slot's outputs and the state behind the commit are compared
 * with the file's; at the end the stream's bytes, and every byte outside the region.  Built and run by tests/test_stream_write_cpu.py.
 *
 * usage: check_stream_write <cases.bin>      (the format: stream_write_cases.write_cases)
 * prints "headers <n> ok <n> differ <n>", "sequences <n> ok <n> differ <n>" and "steps <n>"; exit status 1 on any difference. */
#define PCAMV_HOST_EMU 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pcamv_stream_write.h"

static long n_headers, n_hdiffer, n_seqs, n_sdiffer, n_steps;
static FILE *f;

template <class T> static T get()
{
    T v;
    if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "case file truncated\n"); exit(2); }
    return v;
}
static std::vector<uint8_t> get_bytes(size_t n)
{
    std::vector<uint8_t> v(n);
    if (n && fread(v.data(), 1, n, f) != n) { fprintf(stderr, "case file truncated\n"); exit(2); }
    return v;
}
static pcamv_stream_params_t get_params()
{
    pcamv_stream_params_t P;
    static_assert(sizeof(P) == 12 * 4, "the file holds the twelve members in order");
    const std::vector<uint8_t> v = get_bytes(sizeof(P));
    memcpy(&P, v.data(), sizeof(P));
    return P;
}

static void check_header()
{
    const pcamv_stream_params_t P = get_params();
    pcamv_slice_fields_t F;
    static_assert(sizeof(F) == 12 * 4, "the file holds the twelve members in order");
    const std::vector<uint8_t> v = get_bytes(sizeof(F));
    memcpy(&F, v.data(), sizeof(F));
    const int want_rc = get<int32_t>(), want_bits = get<int32_t>();
    const std::vector<uint8_t> want = get_bytes((size_t)(want_bits + 7) / 8);
    int n0 = -7, n1 = -7;
    const int rc0 = pcamv_slice_header_write(P, F, NULL, &n0);
    int differ = rc0 != want_rc || n0 != want_bits || n0 > PCAMV_SLICE_HDR_MAX_BITS;
    if (!differ) {
        const size_t nb = (size_t)(n0 + 7) / 8;
        uint8_t *block = (uint8_t *)malloc(nb ? nb : 1);                /* (a refused case gets one byte, which must stay as it is) */
        memset(block, 0xA5, nb ? nb : 1);
        const int rc1 = pcamv_slice_header_write(P, F, block, &n1);
        differ |= rc1 != rc0 || n1 != n0 || (nb ? memcmp(block, want.data(), nb) != 0 : block[0] != 0xA5);
        free(block);
    }
    n_headers++;
    if (differ) { if (n_hdiffer < 20) printf("header %ld differs: rc %d (want %d), %d bits (want %d)\n", n_headers - 1, rc0, want_rc, n0, want_bits); n_hdiffer++; }
}

static void check_sequence()
{
    SwsSetup S;
    S.P = get_params();
    static_assert(sizeof(S.W) == 8 * 4, "the file holds the eight members in order");
    { const std::vector<uint8_t> v = get_bytes(sizeof(S.W)); memcpy(&S.W, v.data(), sizeof(S.W)); }
    const long long size = get<int64_t>(), off = get<int64_t>(), cap = get<int64_t>();
    const std::vector<uint8_t> head = get_bytes((size_t)get<int32_t>());
    const int steps = get<int32_t>();
    int differ = sws_setup_ok(S) != 0;
    uint8_t *bytes = (uint8_t *)malloc((size_t)size ? (size_t)size : 1);
    memset(bytes, 0xA5, (size_t)size);
    uint8_t *head_block = (uint8_t *)malloc(head.size() ? head.size() : 1);     /* exact size too: the open reads head[0, head_len) alone */
    if (head.size()) memcpy(head_block, head.data(), head.size());
    const int n = 1 + 2 * (int)(n_seqs % 2), i = (int)(n_seqs % 3) % n;         /* (1, 0), (3, 1), (1, 0), (3, 0), (1, 0), (3, 2), ... */
    const size_t table_bytes = (size_t)n * (SWS_HDR_WORDS * 4 + PCAMV_SLICE_HDR_BYTES);
    int *table = (int *)malloc(table_bytes);
    SwsCtx c;
    long long len = -7;
    sws_open(c, bytes, size, off, cap, head_block, (long long)head.size(), &len);
    const int in = off >= 0 && cap >= 0 && cap <= size && off <= size - cap;    /* (the region lies inside the buffer) */
    for (int k = 0; k < steps; k++) {
        const int qp = get<int32_t>();
        const long long unit_len = get<int64_t>();
        const int want_bits = get<int32_t>();
        const std::vector<uint8_t> want = get_bytes((size_t)(want_bits + 7) / 8);
        const int w_i_frame = get<int32_t>(), w_nal = get<int32_t>();
        const long long w_off = get<int64_t>(), w_cap = get<int64_t>();
        const int w_first = get<int32_t>();
        const long long w_len = get<int64_t>(), w_pic = get<int64_t>(), w_units = get<int64_t>();
        const int w_status = get<int32_t>();
        memset(table, 0xA5, table_bytes);
        const SwsSlot s = sws_slot(S, c, bytes, qp, table, n, i);
        const int *e = table + SWS_HDR_WORDS * i;
        const int at = n * SWS_HDR_WORDS * 4 + i * PCAMV_SLICE_HDR_BYTES;
        differ |= e[0] != at || e[1] != want_bits || e[2] != w_i_frame || e[3] != w_nal || s.off != w_off || s.cap != w_cap || s.first != w_first;
        if (!differ && want.size()) differ |= memcmp((const uint8_t *)table + at, want.data(), want.size()) != 0;
        for (size_t j = 0; j < table_bytes; j++) {                              /* nothing of the table but entry i and the header's bytes in slot i */
            const int own = (j >= (size_t)SWS_HDR_WORDS * 4 * i && j < (size_t)SWS_HDR_WORDS * 4 * (i + 1)) || (j >= (size_t)at && j < (size_t)at + want.size());
            if (!own) differ |= ((const uint8_t *)table)[j] != 0xA5;
        }
        /* the stand-in for the slice writer, with the writers' own test of the place against the buffer */
        long long got_len = 0; int got_status = PCAMV_EINVAL;
        if (s.off >= 0 && s.cap >= 0 && s.cap <= size && s.off <= size - s.cap) {
            const long long fit = unit_len < s.cap ? unit_len : s.cap;
            memset(bytes + s.off, 0x40 + k, (size_t)fit);
            got_status = unit_len > s.cap ? PCAMV_ENOMEM : 0;
            got_len = got_status ? 0 : unit_len;
        }
        int status = -7;
        sws_commit(S, c, s.first, got_len, got_status, &len, &status);
        differ |= len != w_len || c.cur != w_len || c.pic != w_pic || c.units != w_units || status != w_status;
        n_steps++;
    }
    const long long want_len = get<int64_t>();
    const std::vector<uint8_t> stream = get_bytes((size_t)want_len);
    differ |= len != want_len;
    if (!differ && want_len) differ |= memcmp(bytes + off, stream.data(), (size_t)want_len) != 0;
    for (long long j = 0; j < size; j++) if (!in || c.bad || j < off || j >= off + cap) differ |= bytes[j] != 0xA5;
    free(bytes); free(head_block); free(table);
    n_seqs++;
    if (differ) { if (n_sdiffer < 20) printf("sequence %ld differs\n", n_seqs - 1); n_sdiffer++; }
}

int main(int argc, char **argv)
{
    if (argc < 2 || !(f = fopen(argv[1], "rb"))) return 2;
    for (int k = get<int32_t>(); k > 0; k--) check_header();
    for (int k = get<int32_t>(); k > 0; k--) check_sequence();
    if (fgetc(f) != EOF) { fprintf(stderr, "case file has bytes left over\n"); return 2; }
    fclose(f);
    printf("headers %ld ok %ld differ %ld\n", n_headers, n_headers - n_hdiffer, n_hdiffer);
    printf("sequences %ld ok %ld differ %ld\n", n_seqs, n_seqs - n_sdiffer, n_sdiffer);
    printf("steps %ld\n", n_steps);
    return n_hdiffer || n_sdiffer ? 1 : 0;
}
