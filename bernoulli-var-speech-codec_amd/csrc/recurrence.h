// What crosses between the three sources of the BVRNN recurrence: step_plan.hip (the launch-per-layer schedule: plans, their launch and
// their hipGraph cache), flow_launch.hip (the host side of the persistent kernel) and recurrence.hip (the all-frame prologues and the
// drivers).  Host only.  What the other host sources use is in bvc_host.h.
#pragma once
#include "bvc_host.h"

namespace bvc {

// Is this stream being captured?  CAP_FAILED: the query itself failed - the HIP error stays pending for the site to clear
// (hipGetLastError) where it goes on; with `report` it is written to the error text as BVC_HIP_TRY does, for a site that returns BVC_EHIP.
enum Capture { CAP_NONE = 0, CAP_ACTIVE = 1, CAP_FAILED = 2 };
inline Capture capture_state(hipStream_t s, bool report = false) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(s, &cs);
    if (e != hipSuccess) {
        if (report) set_error("%s failed: %s (%s:%d)", "hipStreamIsCapturing(s, &cs)", hipGetErrorString(e), __FILE__, __LINE__);
        return CAP_FAILED;
    }
    return cs == hipStreamCaptureStatusNone ? CAP_NONE : CAP_ACTIVE;
}

// ---- step_plan.hip ------------------------------------------------------------------------------
// One operation of a step: a kernel on the main or the side branch, or an event record / wait that
// forks and joins the two branches (they become graph dependencies under stream capture).
enum { OP_KERNEL = 0, OP_RECORD = 1, OP_WAIT = 2, OP_VBR_CANDIDATES = 3, OP_VBR_SELECT = 4, OP_ENTROPY_DECODE = 5 };   // _VBR_*: the two kernels of k_vbr.hip (v)
                                                                  // _ENTROPY_DECODE: the range decoder of a frame, k_entropy.hip (e)
enum { BR_MAIN = 0, BR_SIDE = 1 };
struct StepNode { int op; int branch; int event; GemmParams p; int epi; VbrStep v; EntropyStep e; };
enum { STEP_ENCODE = 0, STEP_DECODE = 1, STEP_DECODE_PRE = 2, STEP_CONCEAL = 3, STEP_ENCODE_VBR = 4, STEP_ENTROPY = 5 };   // _PRE: phi_z halves of dec.0 / GRU arrive pre-computed
                                                                  // _CONCEAL: the concealing decoder - the encode step with the prior net in the encoder's place
                                                                  // _VBR: the encode step with K candidate rungs per frame (build_vbr_step)
                                                                  // _ENTROPY: the receive program of the entropy-coded wire - the _CONCEAL step with the
                                                                  //   frame's range decoder behind the code epilogue (`es`)
enum { STEP_KIND_MASK = 0xF, STEP_FOLD = 0x10, STEP_RUNGS_SHIFT = 8 };   // | STEP_FOLD: the folded hop (step_fold); | K << STEP_RUNGS_SHIFT: the rungs of a
                                                                  // _VBR step (part of the graph-cache key: the candidate launches have K * B rows)
std::vector<StepNode> build_step(const bvc_model *m, const Workspace &w, int B, int kind_and_fold, const EntropyStep *es = nullptr);
std::vector<StepNode> build_vbr_step(const bvc_model *m, const Workspace &w, const VbrWorkspace &vw, int B, int nrungs);
// the states of one taped frame of BVRNN.forward, fragment-packed [mt16][H]: [0] the teacher-forced chain h, [1] the generated-feature chain h2
struct ForwardTape { float *h_in[2], *h_out[2]; };
std::vector<StepNode> build_forward_step(const bvc_model *m, const Workspace &w, int B, int sel, bool greedy, bool update_h, bool update_h2,
                                         const ForwardTape *tape = nullptr);
int count_kernels(const std::vector<StepNode> &plan);
int step_fold(const bvc_model *m, bool encode);
// probes: the plan's kernels carry in-kernel probes (the buffer is sized and cleared for steps_nodes kernels per step)
int begin_call(const bvc_model *m, const Workspace &w, const CallDesc &v, int steps_nodes, bool probes, hipStream_t s);
int launch_steps(const bvc_model *m, const std::vector<StepNode> &plan, const Workspace &w, int nsteps, hipStream_t s, hipStream_t side);
int run_recurrence(const bvc_model *m, const Workspace &w, void *ws_base, int B, int64_t T, int kind, const std::vector<StepNode> &plan,
                   hipStream_t s);

// ---- flow_launch.hip ----------------------------------------------------------------------------
int flow_chains(const bvc_model *m, int B, hipStream_t s);
int mark_call_end(hipStream_t s);
int run_flow(const bvc_model *m, const Workspace &w, bool encode, int chains, const float *d_h0, int B, int64_t T, const float *d_bits,
             float *d_codes, float *d_prob, float *d_all_h, float *d_mel, float *d_hT, hipStream_t s, const float *d_codes_in = nullptr);

// ---- recurrence.hip -----------------------------------------------------------------------------
int decode_epilogue(const bvc_model *m, const float *keep, int B, int64_t T, float *d_mel, hipStream_t s);

}  // namespace bvc
