// hx_sweep_plan.h -- how the maps of one hx_map2alm_multi / hx_map2alm_list call are cut into sweeps.  Host code without any
// GPU dependency: hx_map2alm.hip queues what this returns, tests/csrc/test_sweep_plan.cpp pins it.
#pragma once
#include <algorithm>
#include <vector>

namespace hx {

// components [c0, c0 + nb) of job `job` as one analysis sweep; stream: its rings are uploaded and transformed slab by slab
struct Sweep { int job, c0, nb; bool stream; };

// staged[j]: the maps of job j go through the staging buffers (host maps, or components in separate arrays);
// next_batch(spin, remaining): components of the sweep that costs least per map; can_stream(spin, nb): such a sweep can run as a
// StreamSweep (asked for staged jobs only).
// A staged sweep that cannot be streamed (the small batches of the vector-unit kernels) is uploaded whole, at most 5 spin-2
// fields / 8 spin-0 maps at a time, and the LAST sweep of the call, if it is of that kind, is halved until it holds at most two
// units: nothing overlaps the transform behind the last upload.  Jobs whose maps are resident are cut by next_batch alone.
template <class NextBatch, class CanStream>
std::vector<Sweep> plan_sweeps(int njobs, const int *spins, const int *ncomps, const std::vector<bool> &staged, NextBatch next_batch, CanStream can_stream)
{
    std::vector<Sweep> sweeps;
    for (int j = 0; j < njobs; ++j) {
        const int unit = spins[j] ? 2 : 1, cap = spins[j] ? 10 : 8;  // 5 spin-2 fields / 8 spin-0 maps: one full column group each
        for (int c0 = 0; c0 < ncomps[j];) {
            const int left = ncomps[j] - c0;
            int nb = next_batch(spins[j], left);
            const bool stream = staged[j] && can_stream(spins[j], nb);
            if (staged[j] && !stream) {
                nb = std::min(cap, left);
                // spin 2: two even sweeps rather than a full and a small one (a sweep costs ~76 ms before its first column);
                // spin 0: a full group, then the rest -- small spin-0 sweeps run on the vector-unit kernel at 23 ms per map
                if (spins[j] && left > cap && left < 2 * cap) nb = (left / unit + 1) / 2 * unit;
            }
            sweeps.push_back({j, c0, nb, stream});
            c0 += nb;
        }
    }
    while (!sweeps.empty() && staged[sweeps.back().job] && !sweeps.back().stream) {
        Sweep &l = sweeps.back();
        const int unit = spins[l.job] ? 2 : 1, units = l.nb / unit;
        if (units <= 2) break;
        const int first = (units + 1) / 2 * unit;
        const Sweep tail = {l.job, l.c0 + first, l.nb - first, false};
        l.nb = first;
        sweeps.push_back(tail);
    }
    return sweeps;
}

}  // namespace hx
