/* az_search_stop.h -- the decided-move stop: end a temperature-0 search once its move can no longer change.
 *
 * Every move played at temperature 0 is argmax(counts) with a one-hot pi.  Once the most visited root child leads the runner-up by more
 * than the simulations still to come, neither can change any more; with the switch on such a search runs none of its remaining
 * simulations and asks the net for no further leaf row.  The rule, operation by operation, and the argument why it is exact:
 * csrc/az_stop.h.
 *
 * An extension header: it includes az_engine.h, az_engine.h does not include it.  libaz_engine.so exports the entries like every other.
 * The switch is a typed setter, not an az_set_option key.
 *
 * ELIGIBLE MOVES (the switch on, temperature 0, the plain PUCT root):
 *     az_selfplay / az_selfplay_begin    the moves with ply + 1 >= temp_threshold (with a playout cap: of the move's own budget)
 *     az_tree_get_action_prob            the calls with temp == 0
 *     az_reanalyse                       the calls with temp == 0
 *     az_arena, az_tournament            every move
 * Root noise does not matter (it only changes priors).  az_tree_slot_get_action_prob is never affected.
 *
 * THE CONTRACT.  With the switch on, an eligible search that ran i* of its B simulations returns
 *     1. pi, the played or selected move and z bit for bit as the full search of B simulations from the same tree returns them;
 *     2. counts, q, the tree, root_q and root_prior bit for bit as the switch-off search with num_sims = i* leaves them.
 * Later moves of the same game start from a smaller re-used subtree, so whole games DIFFER from switch-off games.  With the switch off,
 * and on every move that is not eligible, everything is bit for bit what it was.
 *
 * REFUSED with AZ_ERR_BAD_ARGUMENT while the switch is on, before any search, with an az_last_error that names both sides:
 *     az_selfplay, az_selfplay_begin, az_tree_get_action_prob, az_reanalyse:  num_sim_threads > 1, "selfplay_async" = 1, "gumbel_m" != 0,
 *                                                                             "forced_playouts_k_e6" > 0
 *     az_arena, az_tournament:                                                num_sim_threads > 1
 *
 * SESSION CONTRACT (az_engine.h, next to az_selfplay_begin): a self-play session captures the switch at az_selfplay_begin.
 * az_search_stop_set is refused while a session is open, the session's remaining chunks unchanged; az_search_stop_get and
 * az_search_stop_stats run no device work and are inert beside an open session. */
#ifndef AZ_SEARCH_STOP_H
#define AZ_SEARCH_STOP_H

#include "az_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* on = 0 or 1, state of the engine (0 when it is created); any other value is AZ_ERR_BAD_ARGUMENT */
az_status az_search_stop_set(az_engine* e, int32_t on);
az_status az_search_stop_get(const az_engine* e, int32_t* on);
/* out = {eligible moves, moves stopped early, simulations budgeted on eligible moves, simulations skipped}, summed over the finished
 * calls (a session's chunk is a call) since the engine was created or the counters were last reset; reset != 0 clears them afterwards */
az_status az_search_stop_stats(az_engine* e, uint64_t out[4], int32_t reset);

#ifdef __cplusplus
}
#endif

#endif
