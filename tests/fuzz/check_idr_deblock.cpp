/* The device loop filter of the IDR pictures (csrc/pcamv_idr_deblock.h, what k_idr_deblock runs) on the CPU in the scalar form of SP_LANES,
 * under AddressSanitizer + UBSan when tests/test_idr_deblock_cpu.py builds it: every picture is filtered macroblock by macroblock in the
 * order of the kernel's launches -- anti-diagonal d = x + 2 y after anti-diagonal, the macroblocks of a diagonal once from the top and
 * once from the bottom, since the device runs them in any order -- on planes that are heap blocks of exactly the picture's size, so that
 * an access outside the picture is a report, with the wave's working memory a heap block of exactly its size.  The result of either
 * direction must equal the library's sequential definition pcamv_gpu_deblock_intra_picture (csrc/pcamv_mvsyntax.h), which shares no code
 * and no table with the header under test.
 *
 * Shapes 1x1, 2x1, 1x2, 2x2, 3x3, 6x5, 9x4 macroblocks; every QP 0 .. 51 with chroma offsets -3, 0, +4; noise, steps (one flat value per
 * macroblock, a little noise), ramps and 0 / 255 checkerboards.  No arguments.  Prints "cases <n> bad <n> changed <n> launches_ok <0|1>"
 * and, for a case that fails, "bad <shape> <qp> <offset> <picture> <direction>"; exit status 1 on any failure. */
#include "slice_write_cavlc_host.h"
#include "pcamv_idr_deblock.h"
#include "pcamv_mvsyntax.h"
#include <stdio.h>
#include <random>
#include <vector>

static const int qpc_tab[52] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
                                29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39};

static void picture(int kind, int mb_w, int mb_h, std::mt19937 &rng, std::vector<uint8_t> pl[3])
{
    for (int c = 0; c < 3; c++) {
        const int n = c ? 8 : 16, w = n * mb_w, h = n * mb_h;
        pl[c].assign((size_t)w * h, 0);
        std::vector<int> level((size_t)mb_w * mb_h);
        for (auto &v : level) v = 30 + (int)(rng() % 196);
        const int cell = 1 + (int)(rng() % 4);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                int v;
                if (kind == 0) v = (int)(rng() & 255);
                else if (kind == 1) v = level[(size_t)(y / n) * mb_w + x / n] + (int)(rng() % 7) - 3;
                else if (kind == 2) v = 20 + (c == 2 ? 200 - (x + 2 * y) : x + 2 * y) * (c ? 2 : 1) / 2 + (int)(rng() % 3);
                else v = 255 * (((x / cell) + (y / cell)) & 1);
                pl[c][(size_t)y * w + x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
            }
    }
}

int main()
{
    static const int shapes[7][2] = {{1, 1}, {2, 1}, {1, 2}, {2, 2}, {3, 3}, {6, 5}, {9, 4}};
    static const int offsets[3] = {-3, 0, 4};
    std::mt19937 rng(17);
    long cases = 0, bad = 0, changed = 0;
    int launches_ok = 1;
    IdbWork *W = (IdbWork *)malloc(sizeof(IdbWork));
    if (!W) return 2;
    for (const auto &s : shapes) {
        const int mb_w = s[0], mb_h = s[1];
        /* every macroblock lies on exactly one of the diagonals the launcher walks */
        std::vector<int> seen((size_t)mb_w * mb_h, 0);
        for (int d = 0; d < idb_n_diag(mb_w, mb_h); d++) {
            int y_lo, y_hi;
            idb_diag_rows(d, mb_w, mb_h, &y_lo, &y_hi);
            for (int y = y_lo; y <= y_hi; y++) {
                const int x = d - 2 * y;
                if (x < 0 || x >= mb_w || y < 0 || y >= mb_h) launches_ok = 0; else seen[(size_t)y * mb_w + x]++;
            }
        }
        for (int v : seen) if (v != 1) launches_ok = 0;
        for (int kind = 0; kind < 4; kind++) {
            std::vector<uint8_t> src[3];
            picture(kind, mb_w, mb_h, rng, src);
            for (int qp = 0; qp < 52; qp++)
                for (int off : offsets) {
                    const int qi = qp + off;
                    std::vector<uint8_t> want[3] = {src[0], src[1], src[2]};
                    if (pcamv_gpu_deblock_intra_picture(want[0].data(), want[1].data(), want[2].data(), mb_w, mb_h, qp, off)) return 2;
                    changed += want[0] != src[0] || want[1] != src[1] || want[2] != src[2];
                    for (int rev = 0; rev < 2; rev++) {
                        IdbPic P;
                        for (int c = 0; c < 3; c++) {
                            P.rec[c] = (uint8_t *)malloc(src[c].size());
                            if (!P.rec[c]) return 2;
                            memcpy(P.rec[c], src[c].data(), src[c].size());
                        }
                        P.mb_w = mb_w; P.mb_h = mb_h; P.qp = qp; P.qpc = qpc_tab[qi < 0 ? 0 : qi > 51 ? 51 : qi];
                        for (int d = 0; d < idb_n_diag(mb_w, mb_h); d++) {
                            int y_lo, y_hi;
                            idb_diag_rows(d, mb_w, mb_h, &y_lo, &y_hi);
                            for (int k = 0; k <= y_hi - y_lo; k++) {
                                const int y = rev ? y_hi - k : y_lo + k;
                                idr_deblock_mb(*W, P, d - 2 * y, y);
                            }
                        }
                        int same = 1;
                        for (int c = 0; c < 3; c++) same &= !memcmp(P.rec[c], want[c].data(), want[c].size());
                        if (!same) { bad++; printf("bad %dx%d %d %d %d %d\n", mb_w, mb_h, qp, off, kind, rev); }
                        for (int c = 0; c < 3; c++) free(P.rec[c]);
                        cases++;
                    }
                }
        }
    }
    free(W);
    printf("cases %ld bad %ld changed %ld launches_ok %d\n", cases, bad, changed, launches_ok);
    return bad || !launches_ok ? 1 : 0;
}
