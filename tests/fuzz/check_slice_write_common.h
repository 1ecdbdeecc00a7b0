/* What check_slice_write.cpp and check_slice_write_cavlc.cpp share: the reader of the case file tests/slice_write_cases.py writes
 * (write_case_file), and the loop over its cases.
 *
 * cases.bin: int32 count, then per case int32 {qp, n_hdr_bits, as_nal, short, nal_byte, blobs} and `blobs` (10) blocks of int64 length +
 * bytes: parameters, source Y U V, the padded reference planes (luma x 4, U, V), records, header bits (packed), expected bytes.
 * Every case writes into a heap block of exactly the expected length minus `short`: with short = 0 it must receive the expected
 * bytes, with 1, 2 or 64 bytes less it must give PCAMV_ENOMEM and length 0.  Include after the writer's *_host.h. */
#ifndef CHECK_SLICE_WRITE_COMMON_H
#define CHECK_SLICE_WRITE_COMMON_H
#include <stdio.h>
#include <vector>

static bool sw_check_read_blob(FILE *f, std::vector<uint8_t> &b)
{
    int64_t n = 0;
    if (fread(&n, 8, 1, f) != 1 || n < 0 || n > ((int64_t)1 << 31)) return false;
    b.resize((size_t)n);
    return !n || fread(b.data(), 1, (size_t)n, f) == (size_t)n;
}

/* rc = write(frame, header bits, n_hdr_bits, nal_byte, as_nal, out, cap, &len) for every case of `path`; prints one line per case
 * "<index> <rc> <len> <expected len> <short>" and a summary, which the Python tests parse; returns the program's exit status: 2 for a
 * file that is not a case file, 1 on any failure, else 0 */
template <class Write> static int sw_check_cases(const char *path, Write write)
{
    long bad = 0, fit = 0, refused = 0;
    FILE *f = fopen(path, "rb");
    if (!f) return 2;
    int32_t count = 0;
    if (fread(&count, 4, 1, f) != 1 || count < 0) return 2;
    for (int k = 0; k < count; k++) {
        int32_t h[6];
        if (fread(h, 4, 6, f) != 6 || h[5] != 10) return 2;
        std::vector<uint8_t> blob[10];
        for (int i = 0; i < 10; i++) if (!sw_check_read_blob(f, blob[i])) return 2;
        if (blob[0].size() != sizeof(pcamv_params_t)) return 2;
        pcamv_params_t p;
        memcpy(&p, blob[0].data(), sizeof(p));
        const size_t n_mb = (size_t)(p.i_width / 16) * (p.i_height / 16);
        if (blob[7].size() != n_mb * sizeof(pcamv_mb_t) || blob[1].size() != (size_t)p.i_width * p.i_height) return 2;
        const SliceHostFrame in = {&p, h[0], {blob[1].data(), blob[2].data(), blob[3].data()}, blob[4].data(), blob[5].data(), blob[6].data(),
                                   (const pcamv_mb_t *)blob[7].data(), NULL, 0};
        const long long want = (long long)blob[9].size(), cap = want - h[3];
        if (cap < 0) return 2;
        uint8_t *out = (uint8_t *)malloc(cap ? (size_t)cap : 1);        /* exact size: any store past the capacity is caught */
        long long len = -1;
        const int rc = write(in, blob[8].data(), h[1], h[4], h[2], out, cap, &len);
        printf("%d %d %lld %lld %d\n", k, rc, len, want, h[3]);
        if (h[3] == 0) { if (rc || len != want || memcmp(out, blob[9].data(), (size_t)want)) bad++; else fit++; }
        else { if (rc != PCAMV_ENOMEM || len != 0) bad++; else refused++; }
        free(out);
    }
    fclose(f);
    printf("fit %ld refused %ld bad %ld\n", fit, refused, bad);
    return bad ? 1 : 0;
}
#endif
