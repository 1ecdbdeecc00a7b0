/*
 * pcamv_param_sets_host.h -- pcamv_gpu_parse_sps, pcamv_gpu_parse_pps, pcamv_gpu_stream_param_sets, pcamv_gpu_parse_slice_header_sets:
 * host code of the product library, no GPU.  Included behind pcamv_mvsyntax.h by the one unit that defines the C ABI and by the test
 * driver tests/fuzz/check_param_sets.cpp.
 */
#ifndef PCAMV_PARAM_SETS_HOST_H
#define PCAMV_PARAM_SETS_HOST_H
#include "pcamv_mvsyntax.h"
/* The parameter sets of a stream: these define what k_pset_unit, k_pset_parse, k_pset_resolve and k_slice_header_sets do on every input
 * (include/pcamv_gpu.h states the rules).  The syntax walk and the resolution are pcamv_param_sets.h's, here over the bit-by-bit reader
 * of pcamv_gpu_parse_slice_header, the units cut by pcamv_gpu_annexb_index and unescaped by pcamv_gpu_nal_to_rbsp. */
#include "pcamv_param_sets.h"
namespace mvsyntax {
struct PsHostBits {
    HdrBits b;
    uint32_t u(int n) { return b.u(n); }
    uint64_t ue() { return b.ue(); }
    long long se() { return (long long)b.se(); }
    int failed() const { return b.bad; }
    long long at() const { return (long long)b.pos; }
};
}
extern "C" int pcamv_gpu_parse_sps(const uint8_t *rbsp, size_t len, pcamv_sps_t *out)
{
    if (!out) return PCAMV_EINVAL;
    memset(out, 0, sizeof(*out));
    if ((!rbsp && len) || len > ((size_t)1 << 40)) return PCAMV_EINVAL;
    mvsyntax::PsHostBits B = {{rbsp, (uint64_t)len * 8, 0, 0}};
    const int rc = ps_read_sps(B, *out);
    if (rc) memset(out, 0, sizeof(*out));
    return rc;
}
extern "C" int pcamv_gpu_parse_pps(const uint8_t *rbsp, size_t len, pcamv_pps_t *out)
{
    if (!out) return PCAMV_EINVAL;
    memset(out, 0, sizeof(*out));
    if ((!rbsp && len) || len > ((size_t)1 << 40)) return PCAMV_EINVAL;
    long long last_one = -1;                                                    /* rbsp_stop_one_bit, found bit by bit */
    for (size_t i = 0; i < len * 8; i++) if ((rbsp[i >> 3] >> (7 - (i & 7))) & 1) last_one = (long long)i;
    mvsyntax::PsHostBits B = {{rbsp, (uint64_t)len * 8, 0, 0}};
    const int rc = ps_read_pps(B, last_one, *out);
    if (rc) memset(out, 0, sizeof(*out));
    return rc;
}
extern "C" int pcamv_gpu_stream_param_sets(const uint8_t *bytes, size_t len, pcamv_param_sets_t *out)
{
    if (!out) return PCAMV_EINVAL;
    memset(out, 0, sizeof(*out));
    out->status = PCAMV_EINVAL;
    if (!bytes && len) return PCAMV_EINVAL;
    const size_t cap = len / 3 + 1;
    pcamv_unit_t *units = (pcamv_unit_t *)malloc(cap * sizeof(pcamv_unit_t));
    PsRec *rec = (PsRec *)calloc(PCAMV_PSET_UNITS_MAX, sizeof(PsRec));
    uint8_t *rbsp = (uint8_t *)malloc(PCAMV_PSET_UNIT_BYTES);
    int64_t nu = 0, ns = 0;
    int rc = units && rec && rbsp ? pcamv_gpu_annexb_index(bytes, len, units, cap, &nu, &ns) : PCAMV_ENOMEM;
    if (!rc) {
        long long count = 0;
        for (int64_t i = 0; i < nu; i++) {
            const pcamv_unit_t &u = units[i];
            const int type = u.nal_header & 31;
            if (u.nal_header < 0 || (type != 7 && type != 8)) continue;
            if (count < PCAMV_PSET_UNITS_MAX) {
                PsRec &r = rec[count];
                r.type = type;
                size_t n = 0;
                if (u.len > PCAMV_PSET_UNIT_BYTES) r.code = PCAMV_EUNSUP;
                else r.code = pcamv_gpu_nal_to_rbsp(bytes + u.off, (size_t)u.len, rbsp, &n, NULL, NULL);
                if (!r.code) r.code = type == 7 ? pcamv_gpu_parse_sps(rbsp, n, &r.sps) : pcamv_gpu_parse_pps(rbsp, n, &r.pps);
            }
            count++;
        }
        ps_resolve(rec, count, 0, 0, 0, out);
        rc = out->status;
    }
    free(units); free(rec); free(rbsp);
    return rc;
}
extern "C" int pcamv_gpu_parse_slice_header_sets(const uint8_t *rbsp, size_t len, int nal_header, const pcamv_param_sets_t *sets, int64_t *start_bit,
                                                 int32_t *slice_qp, int32_t *frame_num, int32_t *entropy_cabac)
{
    if (start_bit) *start_bit = -1;
    if (slice_qp) *slice_qp = -1;
    if (frame_num) *frame_num = -1;
    if (entropy_cabac) *entropy_cabac = -1;
    if ((!rbsp && len) || !sets || !start_bit || !slice_qp || !frame_num) return PCAMV_EINVAL;
    if (sets->status) return sets->status;
    if (len > ((size_t)1 << 40)) return PCAMV_EINVAL;
    if (nal_header < 0 || (nal_header & 31) != 1) return PCAMV_EUNSUP;
    mvsyntax::HdrBits b = {rbsp, (uint64_t)len * 8, 0, 0};
    uint64_t e = b.ue();                                                        /* first_mb_in_slice */
    if (b.bad) return PCAMV_EINVAL;
    if (e) return PCAMV_EUNSUP;
    e = b.ue();                                                                 /* slice_type */
    if (b.bad) return PCAMV_EINVAL;
    if (e != 0 && e != 5) return PCAMV_EUNSUP;
    e = b.ue();                                                                 /* pps_id */
    if (b.bad) return PCAMV_EINVAL;
    for (int k = 0; k < sets->n_pps && k < PCAMV_PSET_PPS_MAX; k++)
        if ((uint64_t)sets->pps[k].pps_id == e) {
            if (entropy_cabac) *entropy_cabac = sets->pps[k].entropy_cabac;
            return pcamv_gpu_parse_slice_header(rbsp, len, nal_header, &sets->pps[k], start_bit, slice_qp, frame_num);
        }
    return PCAMV_EUNSUP;
}
#endif
