/* The control code of the byte-stream kernels (csrc/pcamv_stream_index.h: k_stream_scan, k_stream_prefix, k_stream_place, k_slice_header)
 * under AddressSanitizer + UBSan on the CPU, with the host form of SP_LANES, against the library's host functions pcamv_gpu_annexb_index
 * and pcamv_gpu_parse_slice_header (csrc/pcamv_mvsyntax.h), stream by stream and header by header.  Every stream is run with its bytes
 * in an exact-size heap block at each of the four alignments mod 4 (the block begins 0 .. 3 bytes before the stream and ends with it);
 * the chunk summaries, the table and the working memory are exact-size heap blocks too.  The chunk scans run in sequence, then the
 * prefix pass, then the placing scans.  The four alignments take turns with the table's form: every unit / the slice units alone, with
 * max_units the full count / half of it (the count must still be the full count, and nothing past the table may be written).  Built
 * and run by tests/test_stream_index_cpu.py; the inputs are tests/stream_cases.py's: the ones the GPU test hands to the device afterwards.
 *
 * usage: check_stream_index <cases.bin>
 *   cases.bin: twice { int32 fill byte, n_fillers, fillers[]; int32 n_strings, per string uint8 len + bytes } -- each string behind each
 *   filler is a stream; int32 n_streams, per stream int32 len + bytes; int32 n_headers, per header int32 params[12], nal_header, len +
 *   bytes
 * prints "headers <n> ok <n> differ <n>" and "streams <n> ok <n> differ <n>"; exit status 1 on any difference. */
#define PCAMV_HOST_EMU 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pcamv_host_tables.h"
#include "pcamv_mvsyntax.h"
#include "pcamv_stream_index.h"

static long n_streams, n_sdiffer, n_headers, n_hdiffer;
static SiWork work;

static int run_one(const uint8_t *src, long long len, int all, long long max_units, const std::vector<pcamv_unit_t> &want, long long nu, long long ns)
{
    const long long n_chunks = si_chunks(src, len);
    SiChunk *ch = (SiChunk *)malloc((size_t)n_chunks * sizeof(SiChunk));
    pcamv_unit_t *table = (pcamv_unit_t *)malloc((size_t)max_units * sizeof(pcamv_unit_t));
    memset(table, 0xA5, (size_t)max_units * sizeof(pcamv_unit_t));
    unsigned long long longest = 0;
    const SiTable T = {table, max_units, all, &longest};
    long long gu = -7, gs = -7;
    for (long long c = 0; c < n_chunks; c++) si_scan(work, src, len, c, 0, ch + c, T);
    si_prefix(work, src, len, ch, n_chunks, T, &gu, &gs);
    for (long long c = 0; c < n_chunks; c++) si_scan(work, src, len, c, 1, ch + c, T);
    int differ = gu != nu || gs != ns;
    long long at = 0; unsigned long long want_longest = 0;
    for (size_t k = 0; k < want.size(); k++) {
        if (!all && want[k].kind == PCAMV_UNIT_OTHER) continue;
        if (at < max_units) {
            const pcamv_unit_t &g = table[at];
            differ |= g.off != want[k].off || g.len != want[k].len || g.nal_header != want[k].nal_header || g.kind != want[k].kind;
            if (want[k].kind != PCAMV_UNIT_OTHER && (unsigned long long)want[k].len > want_longest) want_longest = (unsigned long long)want[k].len;
        }
        at++;
    }
    differ |= at != (all ? nu : ns) || longest != want_longest;
    for (long long k = at; k < max_units; k++) for (size_t j = 0; j < sizeof(pcamv_unit_t); j++) differ |= ((const uint8_t *)(table + k))[j] != 0xA5;
    free(ch); free(table);
    return differ;
}

static void check_stream(const std::vector<uint8_t> &s)
{
    const size_t len = s.size(), cap = len / 3 + 1;
    std::vector<pcamv_unit_t> want(cap);
    int64_t nu = 0, ns = 0;
    int differ = pcamv_gpu_annexb_index(s.data(), len, want.data(), cap, &nu, &ns) != 0 || (size_t)nu > cap;
    want.resize((size_t)nu);
    /* the host function against the definition, restated naively: every 00 00 01, the unit behind it up to the next one or the end,
     * trailing zeros off; the kind of a unit is not modelled here (tests/test_stream_host.py pins it) */
    {
        std::vector<size_t> pre;
        for (size_t i = 0; i + 2 < len; i++) if (s[i] == 0 && s[i + 1] == 0 && s[i + 2] == 1) pre.push_back(i);
        differ |= pre.size() != (size_t)nu;
        int64_t slices = 0;
        for (size_t k = 0; k < pre.size() && !differ; k++) {
            size_t b = pre[k] + 3, e = k + 1 < pre.size() ? pre[k + 1] : len;
            while (e > b && s[e - 1] == 0) e--;
            differ |= want[k].off != (int64_t)b || want[k].len != (int64_t)(e - b) || want[k].nal_header != (e > b ? (int)s[b] : -1);
            slices += want[k].kind != PCAMV_UNIT_OTHER;
        }
        differ |= !differ && slices != ns;
    }
    for (int a = 0; a < 4 && !differ; a++) {
        uint8_t *block = (uint8_t *)malloc(len + a);                /* ends with the stream: any read past it is caught */
        memset(block, 0, a);
        if (len) memcpy(block + a, s.data(), len);
        const int all = !(a & 1);
        const long long full = all ? nu : ns;
        differ |= run_one(block + a, (long long)len, all, a & 2 ? full / 2 : full, want, nu, ns);
        free(block);
    }
    n_streams++;
    if (differ) { if (n_sdiffer < 20) { printf("stream differs:"); for (size_t k = 0; k < len && k < 24; k++) printf(" %02x", s[k]); printf(" (%zu bytes)\n", len); } n_sdiffer++; }
}

static void check_header(const pcamv_stream_params_t &P, int nal_header, const std::vector<uint8_t> &r)
{
    int64_t sb = -7; int32_t qp = -7, fn = -7;
    const int rc = pcamv_gpu_parse_slice_header(r.data(), r.size(), nal_header, &P, &sb, &qp, &fn);
    int differ = 0;
    for (int a = 0; a < 4; a++) {
        uint8_t *block = (uint8_t *)malloc(r.size() + a);
        if (r.size()) memcpy(block + a, r.data(), r.size());
        long long gsb = -7; int gqp = -7, gfn = -7;
        const int got = pcamv_slice_header_read(block + a, (long long)r.size(), nal_header, P, &gsb, &gqp, &gfn);
        differ |= got != rc || gsb != sb || gqp != qp || gfn != fn;
        free(block);
    }
    n_headers++;
    if (differ) { if (n_hdiffer < 20) { printf("header differs (host rc %d):", rc); for (size_t k = 0; k < r.size() && k < 16; k++) printf(" %02x", r[k]); printf("\n"); } n_hdiffer++; }
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    work.win = (uint32_t *)malloc(SI_WIN_DWORDS * 4); work.sc = (SiChunk *)malloc(64 * sizeof(SiChunk));
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t count = 0;
    for (int part = 0; part < 2; part++) {
        int32_t h[2];
        if (fread(h, 4, 2, f) != 2 || h[1] < 0 || h[1] > 64) return 2;
        std::vector<int32_t> fillers(h[1]);
        if (h[1] && fread(fillers.data(), 4, h[1], f) != (size_t)h[1]) return 2;
        if (fread(&count, 4, 1, f) != 1 || count < 0) return 2;
        for (int k = 0; k < count; k++) {
            uint8_t n, s[255];
            if (fread(&n, 1, 1, f) != 1 || (n && fread(s, 1, n, f) != n)) return 2;
            for (int32_t fl : fillers) {
                std::vector<uint8_t> u((size_t)fl, (uint8_t)h[0]);
                u.insert(u.end(), s, s + n);
                check_stream(u);
            }
        }
    }
    if (fread(&count, 4, 1, f) != 1 || count < 0) return 2;
    for (int k = 0; k < count; k++) {
        int32_t n;
        if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
        std::vector<uint8_t> u((size_t)n);
        if (n && fread(u.data(), 1, u.size(), f) != u.size()) return 2;
        check_stream(u);
    }
    if (fread(&count, 4, 1, f) != 1 || count < 0) return 2;
    for (int k = 0; k < count; k++) {
        int32_t h[14];
        if (fread(h, 4, 14, f) != 14 || h[13] < 0) return 2;
        pcamv_stream_params_t P;
        static_assert(sizeof(P) == 12 * 4, "the file holds the twelve members in order");
        memcpy(&P, h, sizeof(P));
        std::vector<uint8_t> r((size_t)h[13]);
        if (h[13] && fread(r.data(), 1, r.size(), f) != r.size()) return 2;
        check_header(P, h[12], r);
    }
    fclose(f);
    free(work.win); free(work.sc);
    printf("headers %ld ok %ld differ %ld\n", n_headers, n_headers - n_hdiffer, n_hdiffer);
    printf("streams %ld ok %ld differ %ld\n", n_streams, n_streams - n_sdiffer, n_sdiffer);
    return n_sdiffer || n_hdiffer ? 1 : 0;
}
