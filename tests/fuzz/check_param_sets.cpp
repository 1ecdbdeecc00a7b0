/* The control code of the parameter-set kernels (csrc/pcamv_param_sets.h and the selecting scan of csrc/pcamv_stream_index.h: k_stream_scan /
 * k_stream_prefix / k_stream_place with SI_SEL_PSET, k_pset_unit, k_pset_parse, k_pset_resolve, k_slice_header_sets) under AddressSanitizer
 * + UBSan on the CPU, with the host form of SP_LANES, against the library's host functions pcamv_gpu_stream_param_sets and
 * pcamv_gpu_parse_slice_header_sets (csrc/pcamv_param_sets_host.h), stream by stream and header by header.  Every stream is run with its
 * bytes in an exact-size heap block at each of the four alignments mod 4; the chunk summaries, the table of PCAMV_PSET_UNITS_MAX entries,
 * every unit's slot of PCAMV_PSET_UNIT_BYTES bytes, the records and the working memory are exact-size heap blocks too.  The steps run as the
 * launches do: the chunk scans, the prefix pass, the placing scans; then unit by unit the unescaper and the parser; then the resolver.
 * Built and run by tests/test_param_sets_cpu.py; the inputs are tests/param_set_cases.py's: the ones the GPU test hands to the device.
 *
 * usage: check_param_sets <cases.bin>
 *   cases.bin: int32 n_streams, per stream int32 len + bytes; int32 n_headers, per header a pcamv_param_sets_t, int32 nal_header, len + bytes
 * prints "headers <n> ok <n> differ <n>" and "streams <n> ok <n> differ <n>"; exit status 1 on any difference. */
#define PCAMV_HOST_EMU 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pcamv_host_tables.h"
#include "pcamv_mvsyntax.h"
#include "pcamv_param_sets_host.h"

static long n_streams, n_sdiffer, n_headers, n_hdiffer;
static SiWork work;
static NuWork nu_work;

/* what the launches make of one stream */
static void run_one(const uint8_t *src, long long len, pcamv_param_sets_t *out)
{
    const long long n_chunks = si_chunks(src, len);
    SiChunk *ch = (SiChunk *)malloc((size_t)n_chunks * sizeof(SiChunk));
    pcamv_unit_t *table = (pcamv_unit_t *)malloc(PCAMV_PSET_UNITS_MAX * sizeof(pcamv_unit_t));
    const SiTable T = {table, PCAMV_PSET_UNITS_MAX, 0, NULL, SI_SEL_PSET};
    long long n_units = 0, count = 0;
    for (long long c = 0; c < n_chunks; c++) si_scan(work, src, len, c, 0, ch + c, T);
    si_prefix(work, src, len, ch, n_chunks, T, &n_units, &count);
    for (long long c = 0; c < n_chunks; c++) si_scan(work, src, len, c, 1, ch + c, T);
    const long long have = count < PCAMV_PSET_UNITS_MAX ? count : PCAMV_PSET_UNITS_MAX;
    PsRec *rec = (PsRec *)malloc((size_t)(have ? have : 1) * sizeof(PsRec));
    for (long long j = 0; j < have; j++) {
        const pcamv_unit_t u = table[j];
        uint8_t *slot = (uint8_t *)malloc(PCAMV_PSET_UNIT_BYTES);
        long long rbsp_len = -1; int hdr = -1, first = PCAMV_EINVAL;
        if (u.off >= 0 && u.len >= 1 && u.len <= len && u.off <= len - u.len) {            /* k_pset_unit */
            if (u.len > PCAMV_PSET_UNIT_BYTES) { first = PCAMV_EUNSUP; hdr = u.nal_header; }
            else first = pcamv_nal_unescape(nu_work, src + u.off, u.len, slot, &rbsp_len, &hdr);
        }
        if (first || rbsp_len < 0 || rbsp_len > PCAMV_PSET_UNIT_BYTES) {                    /* k_pset_parse */
            memset(&rec[j], 0, sizeof(PsRec));
            rec[j].code = first ? first : PCAMV_EINVAL; rec[j].type = hdr < 0 ? 0 : hdr & 31;
        } else {
            uint8_t *exact = (uint8_t *)malloc((size_t)(rbsp_len ? rbsp_len : 1));          /* the parser reads nothing behind the RBSP */
            memcpy(exact, slot, (size_t)rbsp_len);
            ps_parse_unit(exact, rbsp_len, hdr, rec + j);
            free(exact);
        }
        free(slot);
    }
    ps_resolve(rec, count, 0, 0, 0, out);                                                   /* k_pset_resolve */
    free(rec); free(table); free(ch);
}

static void check_stream(const std::vector<uint8_t> &s)
{
    pcamv_param_sets_t want;
    memset(&want, 0x5a, sizeof(want));
    const int rc = pcamv_gpu_stream_param_sets(s.data(), s.size(), &want);
    int differ = rc != want.status;
    for (int a = 0; a < 4; a++) {
        uint8_t *block = (uint8_t *)malloc(s.size() + a);           /* ends with the stream: any read past it is caught */
        memset(block, 0, a);
        if (s.size()) memcpy(block + a, s.data(), s.size());
        pcamv_param_sets_t got;
        memset(&got, 0xa5, sizeof(got));
        run_one(block + a, (long long)s.size(), &got);
        differ |= memcmp(&got, &want, sizeof(got)) != 0;
        free(block);
    }
    n_streams++;
    if (differ) { if (n_sdiffer < 20) { printf("stream differs (host status %d):", want.status); for (size_t k = 0; k < s.size() && k < 24; k++) printf(" %02x", s[k]); printf(" (%zu bytes)\n", s.size()); } n_sdiffer++; }
}

static void check_header(const pcamv_param_sets_t &T, int nal_header, const std::vector<uint8_t> &r)
{
    int64_t sb = -7; int32_t qp = -7, fn = -7, mode = -7;
    const int rc = pcamv_gpu_parse_slice_header_sets(r.data(), r.size(), nal_header, &T, &sb, &qp, &fn, &mode);
    int differ = 0;
    for (int a = 0; a < 4; a++) {
        uint8_t *block = (uint8_t *)malloc(r.size() + a);
        if (r.size()) memcpy(block + a, r.data(), r.size());
        long long gsb = -7; int gqp = -7, gfn = -7, gmode = -7;
        const int got = pcamv_slice_header_read_sets(block + a, (long long)r.size(), nal_header, T, -1, &gsb, &gqp, &gfn, &gmode);
        differ |= got != rc || gsb != sb || gqp != qp || gfn != fn || gmode != mode;
        /* the context's entropy mode: the entry's own changes nothing, the other one refuses exactly the headers that reached an entry */
        if (gmode >= 0) {
            const int same = pcamv_slice_header_read_sets(block + a, (long long)r.size(), nal_header, T, gmode, &gsb, &gqp, &gfn, &gmode);
            differ |= same != rc || gsb != sb || gqp != qp || gfn != fn;
            const int other = pcamv_slice_header_read_sets(block + a, (long long)r.size(), nal_header, T, !mode, &gsb, &gqp, &gfn, &gmode);
            differ |= other != PCAMV_EUNSUP || gsb != -1 || gqp != -1 || gfn != -1;
        }
        free(block);
    }
    n_headers++;
    if (differ) { if (n_hdiffer < 20) { printf("header differs (host rc %d):", rc); for (size_t k = 0; k < r.size() && k < 16; k++) printf(" %02x", r[k]); printf("\n"); } n_hdiffer++; }
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    work.win = (uint32_t *)malloc(SI_WIN_DWORDS * 4); work.sc = (SiChunk *)malloc(64 * sizeof(SiChunk));
    nu_work.win = (uint32_t *)malloc(NU_WIN_DWORDS * 4); nu_work.out = (uint32_t *)malloc(NU_OUT_DWORDS * 4);
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t count = 0;
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
        pcamv_param_sets_t T;
        int32_t h[2];
        if (fread(&T, sizeof(T), 1, f) != 1 || fread(h, 4, 2, f) != 2 || h[1] < 0) return 2;
        std::vector<uint8_t> r((size_t)h[1]);
        if (h[1] && fread(r.data(), 1, r.size(), f) != r.size()) return 2;
        check_header(T, h[0], r);
    }
    fclose(f);
    free(work.win); free(work.sc); free(nu_work.win); free(nu_work.out);
    printf("headers %ld ok %ld differ %ld\n", n_headers, n_headers - n_hdiffer, n_hdiffer);
    printf("streams %ld ok %ld differ %ld\n", n_streams, n_streams - n_sdiffer, n_sdiffer);
    return n_sdiffer || n_hdiffer ? 1 : 0;
}
