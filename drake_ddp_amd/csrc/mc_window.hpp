// The window arithmetic of an on-device Monte-Carlo run (h_policy.hip: run_policy_mc): how many groups of 64 samples a pass takes, and
// how many passes the run makes.  Plain integers and no HIP include, so that a host-only program can include it
// (tests/test_mc_window.py).
#pragma once
#include <algorithm>
#include <cstddef>

namespace mi_host {

constexpr size_t kMcWindowBytes = 64u << 20;      // what the partials and the optional sample buffers of one pass may take
constexpr unsigned long long kMcEventPairs = 32;  // event pairs a handle keeps for the passes of a run
constexpr size_t kMcTrajWindowBytes = (size_t)1 << 30;   // ... and the trajectory windows of a run that observes envelopes or a box (at least one group)

struct McWindow { unsigned long long k, passes; };     // groups per pass, passes

// G groups of B problems' samples; group_bytes: a group's partials and sample buffers; traj_group_bytes: its trajectories when the run
// observes any (0: none), under a cap of their own; forced_k > 0 (MI_ILQR_MC_PASS_GROUPS) replaces what the caps allow.  Whatever it
// is, a pass holds at least one group, no more than there are, and no more than keep k * B within 31 bits.
static inline McWindow mc_window(unsigned long long G, size_t B, size_t group_bytes, size_t traj_group_bytes, int forced_k,
                                 size_t window_cap = kMcWindowBytes, size_t traj_cap = kMcTrajWindowBytes) {
  unsigned long long k = std::max<unsigned long long>(1, window_cap / group_bytes);
  if (traj_group_bytes) k = std::min(k, std::max<unsigned long long>(1, traj_cap / traj_group_bytes));
  if (forced_k > 0) k = (unsigned long long)forced_k;
  k = std::min(std::min(k, G), std::max<unsigned long long>(1, 0x7fffffffull / B));
  return {k, (G + k - 1) / k};
}

}  // namespace mi_host
