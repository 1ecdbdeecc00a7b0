/*
 * pcamv_rate.hip.h -- a QP per context on the device and the rate controller (gfx950), launched by pcamv_gpu.hip only; the control
 * code is pcamv_rate.h.
 *
 *   k_frame_qp      behind a descriptor upload: one wavefront per context with a QP in force, its row into the pushed descriptor
 *   k_rate_update   behind k_stream_commit: one lane per context, the rule of pcamv_gpu_rate_update on the stream's new length
 *   k_rate_cases    the parity probe of the rule: n cases, one lane each
 */
#ifndef PCAMV_RATE_HIP_H
#define PCAMV_RATE_HIP_H
#include "pcamv_slice.hip.h"
#include "pcamv_rate.h"

/* a context's place in a patch launch.  cell: {the QP in force, the status of the step that set it}, NULL: no QP in force, the
 * descriptor stays the host's.  src (a device-QP step's own push alone): the caller's value, which this launch takes into the cell */
struct QpJob { int *cell; const int *src; const uint32_t *rows; };

/* One wavefront per context.  The QP comes out of the cell (or, in the step that sets it, out of the caller's array and into the cell,
 * clamped, with the status) through one lane, and is the same for all lanes by readfirstlane; then lane l moves dword l of the row. */
static __global__ void __launch_bounds__(64) k_frame_qp(FrameDev *__restrict__ Fs, const QpJob *__restrict__ jobs)
{
    const QpJob j = jobs[blockIdx.x];
    if (!j.cell) return;
    const int l = threadIdx.x;
    int qp = j.src ? *j.src : j.cell[0];
    if (j.src) {
        int outside;
        qp = qprow_clamp(qp, &outside);
        if (l == 0) { j.cell[0] = qp; j.cell[1] = outside ? PCAMV_EINVAL : 0; }
    }
    qp = __builtin_amdgcn_readfirstlane(qp);
    qprow_put((uint32_t *)(void *)&Fs[blockIdx.x], j.rows, qp, l);
}

struct RateJobs {
    pcamv_rate_params_t P;
    pcamv_rate_state_t *state;      /* [n] */
    int *qp;                        /* [n] the controller's cells: what step_rate hands to the step */
    const SwsCtx *ctx; const int *status;
    int n, open;
};
static __global__ void __launch_bounds__(64) k_rate_update(const RateJobs J)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= J.n) return;
    pcamv_rate_state_t s;
    if (J.open) pcamv_rate_open(&J.P, &s, J.ctx[i].cur);
    else { s = J.state[i]; pcamv_rate_step(&J.P, &s, J.ctx[i].cur, J.status[i]); }
    J.state[i] = s; J.qp[i] = s.qp;
}
static __global__ void __launch_bounds__(64) k_rate_cases(const pcamv_rate_params_t *__restrict__ P, pcamv_rate_state_t *__restrict__ state,
                                                          const long long *__restrict__ len, const int *__restrict__ status, int n, int *__restrict__ d)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    pcamv_rate_state_t s = state[i];
    const pcamv_rate_params_t p = P[i];
    d[i] = pcamv_rate_step(&p, &s, len[i], status[i]);
    state[i] = s;
}
#endif
