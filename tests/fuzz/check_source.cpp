/*
 * check_source.cpp -- TEST-ONLY host build of the control code of k_source_feed (csrc/pcamv_source.h: src_check, src_item_lane and
 * what it calls), a loop over work items and lanes standing in for the launch, in the kernel's own order: for every picture, items
 * 0 .. 2 mb_h - 1, lanes 0 .. 63.  Built with -fsanitize=address,undefined.  The clip ends where its heap block ends (and begins
 * where it begins when the base is 0 modulo 16: other bases are reached by an offset into the block; the code under test only ever
 * adds to the clip's address), and each destination plane is a heap block of exactly its size, so a byte read behind the last sample
 * or written outside a plane stops the program.
 *
 * The grid of tests/source_cases.py, taken further: the shapes 1x1, 2x1, 1x2, 3x3, 11x9 (and 8x4 / 9x4 for rows of one 128-byte
 * line and a little more); per shape the paddings 0 .. 14 of the last macroblock in both directions (0, 2, 6, 14 for the larger
 * shapes); the four formats; both line orders; tight, odd-pitched and odd-offset layouts; the clip's base at every address modulo
 * 16.  Every picture is compared, byte for byte, with src_picture_naive, the definition, and the definition with a restatement here
 * that shares nothing with the header.  A census counts the cells (format, flip, alignment class of a luma line's address: 16, 8, 4,
 * 2, 1, padding class to the right: none, some, 14, padding class below): every one of the 360 must have been hit.
 *
 * usage: check_source ; prints "pictures N ok N" and "census 360 hit 360"
 */
#define PCAMV_HOST_EMU
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pcamv_source.h"

static unsigned long long lcg_state = 1;
static unsigned rnd() { lcg_state = lcg_state * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)(lcg_state >> 33); }

static int census[4][2][5][3][3];
static int pad_class(int pad) { return pad == 0 ? 0 : pad == 14 ? 2 : 1; }

/* the layouts of tests/source_cases.py */
static void layout(pcamv_source_t *S, int kind)
{
    const int pairs = S->format >= PCAMV_SRC_NV12, planes = pairs ? 2 : 3;
    long long at = kind == 2 ? 3 : 0;
    for (int k = 0; k < 3; k++) { S->plane_off[k] = 0; S->pitch[k] = 0; }
    for (int k = 0; k < planes; k++) {
        const long long line = k == 0 || pairs ? S->width : S->width / 2, lines = S->height >> !!k;
        S->pitch[k] = kind == 0 ? line : kind == 1 ? ((line + 7) | 1) : line + 6;
        if (kind == 2) at |= 1;
        S->plane_off[k] = at;
        at += S->pitch[k] * lines + (kind == 2 ? 5 : 0);
    }
    S->picture_stride = kind == 0 ? at : at | 1;
}

/* the rule, restated: sample (x, y) of coded plane i */
static uint8_t sample(const pcamv_source_t *S, const uint8_t *pic, int i, int x, int y)
{
    const int w = S->width >> !!i, h = S->height >> !!i;
    if (x > w - 1) x = w - 1;
    if (y > h - 1) y = h - 1;
    if (S->flags & PCAMV_SRC_VFLIP) y = h - 1 - y;
    switch (S->format) {
    case PCAMV_SRC_I420: return pic[S->plane_off[i] + y * S->pitch[i] + x];
    case PCAMV_SRC_YV12: { const int k = i == 1 ? 2 : i == 2 ? 1 : 0; return pic[S->plane_off[k] + y * S->pitch[k] + x]; }
    case PCAMV_SRC_NV12: return i == 0 ? pic[S->plane_off[0] + y * S->pitch[0] + x] : pic[S->plane_off[1] + y * S->pitch[1] + 2 * x + (i == 2)];
    default: return i == 0 ? pic[S->plane_off[0] + y * S->pitch[0] + x] : pic[S->plane_off[1] + y * S->pitch[1] + 2 * x + (i == 1)];
    }
}

static long long n_pictures = 0, n_ok = 0;

static void run_case(int mb_w, int mb_h, int width, int height, int format, int flip, int kind, int base)
{
    const int pictures = 2;
    pcamv_source_t S;
    memset(&S, 0, sizeof(S));
    S.width = width; S.height = height; S.format = format; S.flags = flip ? PCAMV_SRC_VFLIP : 0;
    layout(&S, kind);
    long long one = 0, count = -1;
    if (src_check(&S, 1LL << 40, mb_w, mb_h, &count) || count < 1) { fprintf(stderr, "a case of the grid was refused\n"); exit(1); }
    /* the bytes of one picture: the smallest clip that holds one */
    long long lo = 0, hi = 1LL << 30;
    while (lo < hi) { const long long mid = (lo + hi) / 2; src_check(&S, mid, mb_w, mb_h, &count); if (count >= 1) hi = mid; else lo = mid + 1; }
    one = lo;
    const long long clip_bytes = (pictures - 1) * S.picture_stride + one;
    src_check(&S, clip_bytes, mb_w, mb_h, &count);
    long long below = -1;
    src_check(&S, clip_bytes - 1, mb_w, mb_h, &below);
    if (count != pictures || below != pictures - 1) { fprintf(stderr, "src_check counts %lld / %lld pictures, not %d / %d\n", count, below, pictures, pictures - 1); exit(1); }
    uint8_t *block = (uint8_t *)malloc((size_t)(base + clip_bytes));
    if ((uintptr_t)block & 15) { fprintf(stderr, "malloc gave a block that is not 16-byte aligned\n"); exit(1); }
    uint8_t *clip = block + base;
    for (long long k = 0; k < clip_bytes; k++) clip[k] = (uint8_t)rnd();
    const size_t ysz = (size_t)256 * mb_w * mb_h;
    for (int t = 0; t < pictures; t++) {
        const uint8_t *pic = clip + t * S.picture_stride;
        uint8_t *got[3], *want[3];
        for (int i = 0; i < 3; i++) { got[i] = (uint8_t *)malloc(i ? ysz / 4 : ysz); want[i] = (uint8_t *)malloc(i ? ysz / 4 : ysz); memset(got[i], 0xA5, i ? ysz / 4 : ysz); }
        for (int item = 0; item < src_items(mb_h); item++)
            for (int lane = 0; lane < 64; lane++) src_item_lane(&S, pic, got, mb_w, mb_h, item, lane);
        src_picture_naive(&S, pic, mb_w, mb_h, want);
        int ok = 1;
        for (int i = 0; i < 3; i++) {
            const int W = 16 * mb_w >> !!i, H = 16 * mb_h >> !!i;
            if (memcmp(got[i], want[i], (size_t)W * H)) ok = 0;
            for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) if (want[i][(size_t)y * W + x] != sample(&S, pic, i, x, y)) ok = 0;
        }
        n_pictures++;
        if (ok) n_ok++;
        else if (n_pictures - n_ok < 5) fprintf(stderr, "%dx%d %dx%d format %d flip %d layout %d base %d picture %d differs\n", mb_w, mb_h, width, height, format, flip, kind, base, t);
        for (int y = 0; y < height; y++)
            census[format][flip][src_align_class(pic + S.plane_off[0] + y * S.pitch[0])][pad_class(16 * mb_w - width)][pad_class(16 * mb_h - height)]++;
        for (int i = 0; i < 3; i++) { free(got[i]); free(want[i]); }
    }
    free(block);
}

int main(void)
{
    static const int SHAPES[][3] = {{1, 1, 1}, {2, 1, 1}, {1, 2, 1}, {3, 3, 0}, {8, 4, 0}, {9, 4, 0}, {11, 9, 0}};       /* (mb_w, mb_h, every padding?) */
    static const int FEW[] = {0, 2, 6, 14}, ALL[] = {0, 2, 4, 6, 8, 10, 12, 14};
    for (size_t s = 0; s < sizeof(SHAPES) / sizeof(SHAPES[0]); s++) {
        const int mb_w = SHAPES[s][0], mb_h = SHAPES[s][1], every = SHAPES[s][2], n = every ? 8 : 4;
        const int *pads = every ? ALL : FEW;
        int turn = 0;
        for (int a = 0; a < n; a++)
            for (int b = 0; b < n; b++)
                for (int format = 0; format < 4; format++)
                    for (int flip = 0; flip < 2; flip++)
                        for (int kind = 0; kind < 3; kind++) {
                            /* the small shapes at every base; the larger ones at four bases in turn, so that all sixteen come round */
                            const int bases = every ? 16 : 4;
                            for (int k = 0; k < bases; k++) run_case(mb_w, mb_h, 16 * mb_w - pads[a], 16 * mb_h - pads[b], format, flip, kind, every ? k : (4 * k + turn) & 15);
                            turn++;
                        }
    }
    int cells = 0, hit = 0;
    for (int f = 0; f < 4; f++) for (int v = 0; v < 2; v++) for (int c = 0; c < 5; c++) for (int px = 0; px < 3; px++) for (int py = 0; py < 3; py++) {
        cells++;
        if (census[f][v][c][px][py]) hit++;
        else fprintf(stderr, "census: format %d flip %d alignment class %d padding %d %d never hit\n", f, v, c, px, py);
    }
    printf("pictures %lld ok %lld\n", n_pictures, n_ok);
    printf("census %d hit %d\n", cells, hit);
    return n_pictures == n_ok && cells == hit ? 0 : 1;
}
