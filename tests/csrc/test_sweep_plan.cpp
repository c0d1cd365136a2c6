// How hx_map2alm_multi / hx_map2alm_list cut the maps of a call into sweeps (hx_sweep_plan.h), on the host.
// Build: g++ -O2 -std=c++17 test_sweep_plan.cpp
#include <cstdio>
#include <vector>
#include "../../heracles_amd/csrc/hx_sweep_plan.h"
using hx::Sweep;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            ++failures;                       \
            printf("FAIL %s: ", name);        \
            printf(__VA_ARGS__);              \
            printf(" (%s)\n", #cond);         \
        }                                     \
    } while (0)

struct Job { int spin, ncomp; bool staged; };
typedef std::vector<std::vector<int>> Lists;  // nb of the sweeps of every job, in order

// stand-ins for analysis_next_batch: at most 12 spin-2 / 16 spin-0 components, or at most 20
static int batch_12_16(int spin, int remaining) { return remaining < (spin ? 12 : 16) ? remaining : (spin ? 12 : 16); }
static int batch_20(int, int remaining) { return remaining < 20 ? remaining : 20; }

template <class NextBatch>
static std::vector<Sweep> run(const char *name, const std::vector<Job> &jobs, NextBatch next_batch, bool streamable, const Lists &expect)
{
    std::vector<int> spins, ncomps;
    std::vector<bool> staged;
    for (const Job &j : jobs) { spins.push_back(j.spin); ncomps.push_back(j.ncomp); staged.push_back(j.staged); }
    const std::vector<Sweep> sw = hx::plan_sweeps((int)jobs.size(), spins.data(), ncomps.data(), staged, next_batch, [&](int spin, int nb) {
        (void)spin; (void)nb;
        return streamable;
    });
    // every job is covered once, in order, in whole units; staged sweeps that are not streamed respect the cap
    Lists got(jobs.size());
    size_t k = 0;
    for (size_t j = 0; j < jobs.size(); ++j) {
        const int unit = jobs[j].spin ? 2 : 1;
        int c0 = 0;
        for (; k < sw.size() && sw[k].job == (int)j; ++k) {
            CHECK(sw[k].c0 == c0, "sweep %zu starts at %d, expected %d", k, sw[k].c0, c0);
            CHECK(sw[k].nb > 0 && sw[k].nb % unit == 0, "sweep %zu holds %d components", k, sw[k].nb);
            CHECK(!sw[k].stream || jobs[j].staged, "sweep %zu of a resident job is streamed", k);
            if (jobs[j].staged && !sw[k].stream) CHECK(sw[k].nb <= (jobs[j].spin ? 10 : 8), "staged sweep %zu holds %d components", k, sw[k].nb);
            c0 += sw[k].nb;
            got[j].push_back(sw[k].nb);
        }
        CHECK(c0 == jobs[j].ncomp, "job %zu: %d of %d components covered", j, c0, jobs[j].ncomp);
    }
    CHECK(k == sw.size(), "%zu sweeps out of job order", sw.size() - k);
    if (!sw.empty() && jobs[sw.back().job].staged && !sw.back().stream)
        CHECK(sw.back().nb / (jobs[sw.back().job].spin ? 2 : 1) <= 2, "last sweep holds %d components", sw.back().nb);
    bool same = got == expect;
    CHECK(same, "sweep lists differ");
    if (!same)
        for (size_t j = 0; j < got.size(); ++j) {
            printf("  job %zu:", j);
            for (int nb : got[j]) printf(" %d", nb);
            printf("\n");
        }
    return sw;
}

int main()
{
    // staged jobs, nothing streamable: cap of 5 fields / 8 maps, even split of a spin-2 tail, the last sweep halved to <= 2 units
    run("spin 2, 14", {{2, 14, true}}, batch_12_16, false, {{8, 4, 2}});
    run("spin 2, 10", {{2, 10, true}}, batch_12_16, false, {{6, 4}});
    run("spin 2, 20", {{2, 20, true}}, batch_12_16, false, {{10, 6, 4}});
    run("spin 0, 11", {{0, 11, true}}, batch_12_16, false, {{8, 2, 1}});
    run("spin 2, 10 + spin 0, 3", {{2, 10, true}, {0, 3, true}}, batch_12_16, false, {{10}, {2, 1}});
    {
        // everything streamable: the sweeps of next_batch, streamed, nothing halved
        const char *name = "streamed spin 2, 20";
        const std::vector<Sweep> sw = run(name, {{2, 20, true}}, batch_20, true, {{20}});
        CHECK(sw.size() == 1 && sw[0].stream, "not one streamed sweep");
    }
    {
        // resident maps: the sweeps of next_batch, none streamed even where a sweep could be, none halved
        const char *name = "resident spin 2, 30";
        for (const Sweep &w : run(name, {{2, 30, false}}, batch_12_16, true, {{12, 12, 6}})) CHECK(!w.stream, "streamed");
        run("resident spin 0, 40", {{0, 40, false}}, batch_12_16, false, {{16, 16, 8}});
    }
    // only the last sweep of the CALL is halved, and only if it is staged and not streamed
    run("resident spin 2, 30 + staged spin 0, 11", {{2, 30, false}, {0, 11, true}}, batch_12_16, false, {{12, 12, 6}, {8, 2, 1}});
    run("staged spin 2, 10 + resident spin 0, 4", {{2, 10, true}, {0, 4, false}}, batch_12_16, false, {{10}, {4}});
    if (failures) printf("%d checks failed\n", failures);
    return failures ? 1 : 0;
}
