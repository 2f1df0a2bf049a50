// so_run_select.h — which persistent-run kernel a launch uses: the one list of instantiations
// and the one function that picks from it.  Plain C++ (no HIP), so a host compiler builds it
// alone (tests/host/run_select_check.cpp pins every choice); so_me.hip attaches the kernels.
#pragma once

namespace so {

// kRunFPipe2P: the frame pipeline with two-pass RC (each tile a pass-1 and a pass-2 task as
// kRunTwoPass; the reference arrives in the landing planes as kRunFPipe, and pass 2 pushes
// the final reconstruction on to the rank encoding the next frame)
constexpr int kRunSingle = 0, kRunStripe = 1, kRunFPipe = 2, kRunTwoPass = 3, kRunFPipe2P = 4;

// One instantiation: p_run_kernel<NW, mode, vbs, hooks, uqp, slot>, or -- the plain one-GPU run
// without hooks on 32-row tiles (!tall) -- p_run_short_kernel<NW, slot>.  `slot` is p_run_kernel's
// ZSKIP parameter: the zero-skip transforms of a plain run, the latency-bound (ballot) lists of a
// uniform-QP VBS run.  `tall`: 48-row tiles (p_run_kernel's kRunHasTall).
struct RunKernelKey {
    int mode;
    bool vbs, hooks, uqp, slot, tall;
};
// (the order only sets the order the kernels are emitted in the code object)
constexpr RunKernelKey kRunKernels[] = {
    // VBS
    {kRunSingle, true, false, false, false, false},
    {kRunSingle, true, true, false, false, false},
    {kRunSingle, true, false, true, false, false},   // mask-built lists
    {kRunSingle, true, true, true, false, false},
    {kRunSingle, true, false, true, true, false},    // the latency-bound twin: ballot-built lists
    {kRunFPipe, true, false, false, false, false},
    {kRunFPipe, true, false, true, false, false},
    // plain
    {kRunSingle, false, false, false, false, true},
    {kRunSingle, false, true, false, false, false},
    {kRunSingle, false, false, false, true, true},
    {kRunSingle, false, false, false, false, false},   // p_run_short_kernel
    {kRunSingle, false, false, false, true, false},    // p_run_short_kernel
    {kRunStripe, false, false, false, false, false},
    {kRunFPipe, false, false, false, false, false},
    {kRunTwoPass, false, false, false, false, false},
    {kRunFPipe2P, false, false, false, false, false},
};
constexpr int kRunKernelCount = sizeof(kRunKernels) / sizeof(kRunKernels[0]);

// refusals of run_kernel_select: the hook options on a run kind with no hook instantiation
// (the caller's error, SO_E_INVALID); a combination no launcher asks for
constexpr int kRunSelectHooks = -1, kRunSelectNone = -2;

constexpr int run_kernel_find(int mode, bool vbs, bool hooks, bool uqp, bool slot, bool tall) {
    for (int i = 0; i < kRunKernelCount; ++i) {
        const RunKernelKey& k = kRunKernels[i];
        if (k.mode == mode && k.vbs == vbs && k.hooks == hooks && k.uqp == uqp && k.slot == slot && k.tall == tall)
            return i;
    }
    return kRunSelectNone;
}

// The kernel of one launch, as an index into kRunKernels (or a refusal).
//   hook_set: SO_OPT_COUNT_SAD_OPS or SO_OPT_TEST_LOSE_FLAG is set (the test-hook instantiation)
//   no_qp_row: no row-QP schedule (VBS then runs its uniform-QP instantiation)
//   zero_skip: SO_OPT_RUN_ZERO_SKIP (the plain one-GPU run's all-zero-wave IDCT skip; not with hooks)
//   tall: the plain one-GPU run's tile choice (p_run_tall_choice); ignored elsewhere
//   latency_bound: a frame has fewer tiles than the launch's grid has slots (the uniform-QP VBS
//                  one-GPU run then takes its ballot-list twin: 1080p VBS GOP 1.433 -> 1.399 ms,
//                  profiles/r06/ab_vbs_ballot_latency.log)
constexpr int run_kernel_select(int mode, bool vbs, bool hook_set, bool no_qp_row, bool zero_skip, bool tall,
                                bool latency_bound) {
    const bool single = mode == kRunSingle;
    if (hook_set && !single) return kRunSelectHooks;
    const bool uqp = vbs && no_qp_row;
    if (hook_set) return run_kernel_find(mode, vbs, true, uqp, false, false);
    if (uqp) return run_kernel_find(mode, true, false, true, single && latency_bound, false);
    if (single && !vbs) return run_kernel_find(mode, false, false, false, zero_skip, tall);
    return run_kernel_find(mode, vbs, false, false, false, false);
}

// p_run_capacity's filter: the instantiations a run of that VBS setting may launch, in one mode
// or (mode < 0) in any -- hook entries included
constexpr bool run_kernel_counts(int i, bool vbs, int mode) {
    return kRunKernels[i].vbs == vbs && (mode < 0 || kRunKernels[i].mode == mode);
}

}  // namespace so
