// Which persistent-run kernel a launch uses (streamoptima_amd/csrc/so_run_select.h), checked on
// the host against a truth table written out below: every combination of run_kernel_select's
// inputs, every table entry reachable, and p_run_capacity's two filters.  All the twins are
// bit-exact, so no GPU test can see a wrong pick: this is where the choice is pinned.
// Built and run by tests/test_host.py (CPU).  Exit status 0 = every choice as listed.
#include "../../streamoptima_amd/csrc/so_run_select.h"

#include <stdio.h>

using namespace so;

constexpr int X = -1;   // any value
struct Row {
    int mode, vbs, hook_set, no_qp_row, zero_skip, tall, latency_bound;   // inputs (0, 1 or X)
    int refusal;                                                           // < 0: refused with it
    RunKernelKey key;                                                      // else this instantiation
};
// p_run_kernel<8, mode, vbs, hooks, uqp, slot>; !tall on a plain hook-free kRunSingle entry is
// p_run_short_kernel<8, slot>
static const Row kTruth[] = {
    // the hook options on a run kind with no hook instantiation: refused
    {kRunStripe, X, 1, X, X, X, X, kRunSelectHooks, {}},
    {kRunFPipe, X, 1, X, X, X, X, kRunSelectHooks, {}},
    {kRunTwoPass, X, 1, X, X, X, X, kRunSelectHooks, {}},
    {kRunFPipe2P, X, 1, X, X, X, X, kRunSelectHooks, {}},
    // one GPU with hooks: the row-QP or the uniform-QP hook kernel; zero-skip, tall, latency ignored
    {kRunSingle, 0, 1, X, X, X, X, 0, {kRunSingle, false, true, false, false, false}},
    {kRunSingle, 1, 1, 0, X, X, X, 0, {kRunSingle, true, true, false, false, false}},
    {kRunSingle, 1, 1, 1, X, X, X, 0, {kRunSingle, true, true, true, false, false}},
    // one GPU, VBS: uniform QP takes the latency twin when latency-bound, else the mask lists
    {kRunSingle, 1, 0, 1, X, X, 1, 0, {kRunSingle, true, false, true, true, false}},
    {kRunSingle, 1, 0, 1, X, X, 0, 0, {kRunSingle, true, false, true, false, false}},
    {kRunSingle, 1, 0, 0, X, X, X, 0, {kRunSingle, true, false, false, false, false}},
    // one GPU, plain: 32-row twin or 48-row tiles, each with and without zero-skip
    {kRunSingle, 0, 0, X, 0, 0, X, 0, {kRunSingle, false, false, false, false, false}},
    {kRunSingle, 0, 0, X, 1, 0, X, 0, {kRunSingle, false, false, false, true, false}},
    {kRunSingle, 0, 0, X, 0, 1, X, 0, {kRunSingle, false, false, false, false, true}},
    {kRunSingle, 0, 0, X, 1, 1, X, 0, {kRunSingle, false, false, false, true, true}},
    // the frame pipeline: plain, VBS with a row-QP schedule, VBS with uniform QP
    {kRunFPipe, 0, 0, X, X, X, X, 0, {kRunFPipe, false, false, false, false, false}},
    {kRunFPipe, 1, 0, 0, X, X, X, 0, {kRunFPipe, true, false, false, false, false}},
    {kRunFPipe, 1, 0, 1, X, X, X, 0, {kRunFPipe, true, false, true, false, false}},
    // stripe and the two-pass kinds: plain only
    {kRunStripe, 0, 0, X, X, X, X, 0, {kRunStripe, false, false, false, false, false}},
    {kRunTwoPass, 0, 0, X, X, X, X, 0, {kRunTwoPass, false, false, false, false, false}},
    {kRunFPipe2P, 0, 0, X, X, X, X, 0, {kRunFPipe2P, false, false, false, false, false}},
    {kRunStripe, 1, 0, X, X, X, X, kRunSelectNone, {}},
    {kRunTwoPass, 1, 0, X, X, X, X, kRunSelectNone, {}},
    {kRunFPipe2P, 1, 0, X, X, X, X, kRunSelectNone, {}},
};

static bool fits(int want, int v) { return want == X || want == v; }
static bool same(const RunKernelKey& a, const RunKernelKey& b) {
    return a.mode == b.mode && a.vbs == b.vbs && a.hooks == b.hooks && a.uqp == b.uqp && a.slot == b.slot &&
           a.tall == b.tall;
}

int main() {
    long bad = 0;
    bool reached[kRunKernelCount] = {};
    if (kRunKernelCount != 16) {
        printf("the table has %d entries, not 16\n", kRunKernelCount);
        ++bad;
    }
    for (int i = 0; i < kRunKernelCount; ++i)
        for (int j = 0; j < i; ++j)
            if (same(kRunKernels[i], kRunKernels[j])) {
                printf("entries %d and %d are the same instantiation\n", j, i);
                ++bad;
            }
    for (int c = 0; c < 5 * 64; ++c) {
        const int mode = c >> 6, vbs = c >> 5 & 1, hk = c >> 4 & 1, nq = c >> 3 & 1, zs = c >> 2 & 1, tall = c >> 1 & 1,
                  lat = c & 1;
        const Row* row = nullptr;
        int nrows = 0;
        for (const Row& r : kTruth)
            if (r.mode == mode && fits(r.vbs, vbs) && fits(r.hook_set, hk) && fits(r.no_qp_row, nq) &&
                fits(r.zero_skip, zs) && fits(r.tall, tall) && fits(r.latency_bound, lat)) {
                row = &r;
                ++nrows;
            }
        if (nrows != 1) {   // the truth table itself: one row per combination
            printf("mode %d vbs %d hooks %d noqp %d zs %d tall %d lat %d: %d truth rows\n", mode, vbs, hk, nq, zs,
                   tall, lat, nrows);
            ++bad;
            continue;
        }
        const int got = run_kernel_select(mode, vbs != 0, hk != 0, nq != 0, zs != 0, tall != 0, lat != 0);
        bool ok;
        if (row->refusal < 0)
            ok = got == row->refusal;
        else {
            ok = got >= 0 && got < kRunKernelCount && same(kRunKernels[got], row->key);
            if (ok) reached[got] = true;
        }
        if (!ok) {
            printf("mode %d vbs %d hooks %d noqp %d zs %d tall %d lat %d: got %d\n", mode, vbs, hk, nq, zs, tall, lat,
                   got);
            ++bad;
        }
    }
    for (int i = 0; i < kRunKernelCount; ++i)
        if (!reached[i]) {
            printf("entry %d is never selected\n", i);
            ++bad;
        }
    // p_run_capacity(vbs, -1): every entry of that VBS setting, hook entries included
    int n[2] = {0, 0};
    for (int v = 0; v < 2; ++v)
        for (int i = 0; i < kRunKernelCount; ++i) n[v] += run_kernel_counts(i, v != 0, -1) ? 1 : 0;
    if (n[0] != 9 || n[1] != 7) {
        printf("capacity filters: %d plain and %d VBS entries, not 9 and 7\n", n[0], n[1]);
        ++bad;
    }
    // and per mode they partition it
    for (int v = 0; v < 2; ++v) {
        int sum = 0;
        for (int m = 0; m < 5; ++m)
            for (int i = 0; i < kRunKernelCount; ++i) sum += run_kernel_counts(i, v != 0, m) ? 1 : 0;
        if (sum != n[v]) {
            printf("capacity filters by mode: %d entries, not %d (vbs %d)\n", sum, n[v], v);
            ++bad;
        }
    }
    printf("%ld mismatches\n", bad);
    return bad ? 1 : 0;
}
