/* TEST-ONLY: tests/emu/libpcamv_slice_write_emu.so -- the device slice writer's control code on the CPU (slice_write_host.h) */
#include "slice_write_host.h"

extern "C" int swx_write(const pcamv_params_t *p, int qp, const uint8_t *fy, const uint8_t *fu, const uint8_t *fv, uint8_t *luma4, uint8_t *cu, uint8_t *cv,
                         const pcamv_mb_t *mbs, const int8_t *flip, int n_flip, const uint8_t *hdr_bits, int n_bits, int i_frame, int nal_byte,
                         int as_nal, long long cap, uint8_t *out, long long *len, uint32_t *hash)
{
    const SwHostFrame in = {p, qp, {fy, fu, fv}, luma4, cu, cv, mbs, flip, n_flip};
    uint8_t *buf = (uint8_t *)malloc(cap > 0 ? (size_t)cap : 1);          /* exactly the capacity, wherever the caller's array ends */
    const int rc = sw_host_write(in, hdr_bits, n_bits, i_frame, nal_byte, as_nal, buf, cap, len, hash);
    if (!rc) memcpy(out, buf, (size_t)*len);
    free(buf);
    return rc;
}

/* the writer's packed-word carrier arithmetic against carrier_slots / carrier_of_block of pcamv_logic.h, over every partitioning:
 * returns the number of (macroblock shape, block) pairs that differ */
extern "C" int swx_carrier_arithmetic_differs(void)
{
    int bad = 0;
    for (int shape = 0; shape < 3 + 256; shape++) {
        const int type = shape < 3 ? PCAMV_P_L0 : PCAMV_P_8x8, partition = shape == 0 ? PCAMV_D_16x16 : shape == 1 ? PCAMV_D_16x8 : shape == 2 ? PCAMV_D_8x16 : PCAMV_D_8x8;
        const int c = shape < 3 ? 0xff : shape - 3;
        const uint8_t sub[4] = {(uint8_t)(c & 3), (uint8_t)((c >> 2) & 3), (uint8_t)((c >> 4) & 3), (uint8_t)((c >> 6) & 3)};
        const uint32_t packed = (uint32_t)sub[0] | (uint32_t)sub[1] << 8 | (uint32_t)sub[2] << 16 | (uint32_t)sub[3] << 24;
        int slots[16];
        const int n = carrier_slots(type, partition, sub, 1, slots);
        for (int i = 0; i < 16; i++) {
            const int s = carrier_of_block(type, partition, sub, i);
            int rank = -1;
            for (int j = 0; j < n; j++) if (slots[j] == s) rank = j;
            if (sw_block_slot(type, partition, packed, i) != s || sw_slot_rank(type, packed, s) != rank) bad++;
        }
    }
    return bad;
}

/* sp_partition of pcamv_slice_parse.h (the partition walk of all four slice coders) as it is, and the embedding stage's carrier_slots
 * of the same macroblock shape (sub: the four sub-partitions, one byte each; returns the count), for the test to set side by side */
extern "C" int swx_partition(int type, int partition, uint32_t sub, int k) { return sp_partition(type, partition, sub, k); }
extern "C" int swx_carrier_slots(int type, int partition, uint32_t sub, int slots[16])
{
    const uint8_t s[4] = {(uint8_t)sub, (uint8_t)(sub >> 8), (uint8_t)(sub >> 16), (uint8_t)(sub >> 24)};
    return carrier_slots(type, partition, s, 1, slots);
}
