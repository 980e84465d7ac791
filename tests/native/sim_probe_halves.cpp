// The probe geometry "32 lanes x 8 samples" (two such slots share a wave on the device, one per half) through the
// lock-step simulator: the per-thread phases of analyze_core.h are the kernel's own, the cross-thread steps are the
// simulator's.  Exports the plan of one slot of at most 256 samples for tests/test_probe_halves_sim.py.
#include "sim_analyze.cpp"

extern "C" int sim_probe_plan_8x32(const int32_t* x, uint32_t n, int zero_run, int partitioning, int force_wide,
                                   lacx::ChannelPlan* out) {
    using G = lacx::Geo<8, 32>;
    static_assert(G::MAXN == 256 && G::SW == 32 && G::NW == 1 && G::W256 == 32 && G::TPG == 8 && G::MAXP == 3,
                  "one 256-sample probe slot in half a wave");
    if (n == 0 || n > (uint32_t)G::MAXN) return -2;
    return run_sim<G>(x, n, zero_run, partitioning, force_wide, out);
}
