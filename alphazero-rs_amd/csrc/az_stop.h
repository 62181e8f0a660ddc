// az_stop.h -- the decided-move stop (include/az_search_stop.h): a temperature-0 search ends once its most visited
// root child leads the runner-up by more than the simulations still to come.  HIP-free apart from the host/device qualifier (AZS_HD, as
// az_playout.h has AZP_HD): the tree kernels, the engine's host code and the g++ programs of the tests compile this text.  Integer
// operations only.
//
// A MOVE is one get_action_prob of one tree with budget B (num_sims; under a playout cap the move's own budget from PlayoutCap.word).
// A move is ELIGIBLE when the feature is on, its temperature is 0 (stop_eligible) and the root rule is plain PUCT.
//
// THE DECISION is taken before every simulation i + 1, i = 0 .. B - 1: after the backup of simulation i (for i = 0, after the root's own
// priors are stored).  n_j = the root children's visit counts exactly as root_policy reads them (a link slot resolved to its canonical
// node, the raw u16); n1 >= n2 = the two largest (n2 = 0 when the root has one child); left = B - i.  The move is DECIDED iff
//     n1 - n2 > left                                                                                     (strict)
// and a decided tree runs none of its `left` simulations.  i = 0 counts: a reused root can be decided before its first simulation.
//
// WHY IT IS EXACT.  The rule rests on ONE PROPERTY of a search with one simulation in flight per tree: a simulation raises exactly one root
// child's N by one and lowers none (a transposition link joins nodes of equal stone count only, so no deeper node is a root child).  Then
// after the `left` simulations the leader still has n1' >= n1 > n2 + left >= every other child's count: the maximum of the final counts is
// unique and is today's leader, so argmax(counts), the one-hot pi and the tie-break draw (never used: one maximum) are the full search's.
// What a stopped search returns:
//   1. pi, the played / selected move and z are bit for bit the full search's from the same tree;
//   2. counts, q, the tree, root_q and root_prior are bit for bit those of the feature-off search with num_sims = i*, the simulations run.
// LATER moves of the same game start from a smaller reused subtree, so whole games DIFFER from feature-off games.
//
// THE WORD.  The lock-step kernels keep a searching tree's move in TreeHead.active (az_tree.h):
//     bit 0 the tree searches | bits 1 .. 29 the simulations the move has left | bit 30 the move was decided | bit 31 the move is eligible
// The playout cap's own word (1 | left << 1) is the same word with the upper bits clear.  A decided tree keeps its `left`: it is what the
// move skipped, read where the move is played or emitted (stop_count).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define AZS_HD __host__ __device__ __forceinline__
#else
#define AZS_HD inline
#endif

namespace az {

constexpr uint32_t STOP_DECIDED_BIT = 0x40000000u, STOP_ELIGIBLE_BIT = 0x80000000u, STOP_LEFT_MASK = 0x1FFFFFFFu;
enum StopStat { SS_ELIGIBLE = 0, SS_STOPPED, SS_BUDGET, SS_SKIPPED, SS_COUNT };     // eligible moves, moves stopped early, simulations budgeted on eligible moves, simulations skipped

// temperature 0: self-play's test of selfplay_move_body (ply + 1 >= temp_threshold); the tree call and az_reanalyse pass INT32_MIN for
// temp == 0 and INT32_MAX otherwise; the arena and the tournament INT32_MIN
AZS_HD bool stop_eligible(int32_t ply, int32_t temp_threshold) { return (int64_t)ply + 1 >= (int64_t)temp_threshold; }
// the word a searching tree's move starts with
AZS_HD uint32_t stop_word(uint32_t budget, bool eligible) { return 1u | ((budget & STOP_LEFT_MASK) << 1) | (eligible ? STOP_ELIGIBLE_BIT : 0u); }
AZS_HD uint32_t stop_left(uint32_t word) { return (word >> 1) & STOP_LEFT_MASK; }
// the two largest of the counts seen so far (start from n1 = n2 = 0)
AZS_HD void stop_top2(uint32_t& n1, uint32_t& n2, uint32_t n) {
    if (n > n1) { n2 = n1; n1 = n; }
    else if (n > n2) n2 = n;
}
AZS_HD bool stop_decided(uint32_t n1, uint32_t n2, uint32_t left) { return n1 - n2 > left; }
// the rule over a root's counts in slot order
AZS_HD bool stop_decided_counts(const uint32_t* n, int nchild, uint32_t left) {
    uint32_t n1 = 0u, n2 = 0u;
    for (int j = 0; j < nchild; ++j) stop_top2(n1, n2, n[j]);
    return stop_decided(n1, n2, left);
}

}  // namespace az
