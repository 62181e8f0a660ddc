/* az_reanalyse.h -- re-search a window of stored positions with the current net.
 *
 * Every tuple of an older self-play window still carries the pi of the weaker net that played it.  az_reanalyse searches n stored
 * positions with a model as it is NOW and returns what a fresh search of each says: the policy target, and next to it the root value and
 * the root's stored priors that az_samples_blend_z and az_samples_surprise take.  No game is played.
 *
 * An extension header: it includes az_engine.h, az_engine.h does not include it.  libaz_engine.so exports the entry like every other.
 *
 * THE CONTRACT.  Row i of pi, counts and q is bit for bit what az_tree_get_action_prob returns for a ONE-tree az_tree
 *     created with the same num_sims, num_sim_threads, max_depth, cpuct, model_id and reserve,
 *     after az_tree_reset(t, &states[i]),
 *     called with the same temp and seed and first_game_id = game_ids[i]        (game_ids == NULL: first_game_id + i),
 * under the engine's options as they stand: root noise, forced playouts with "policy_prune" and "gumbel_m" apply exactly as they apply to
 * that call (the playout cap never does, as in the tree calls); "eval_mirror", "net_fp8" and a model's own class select the net's answers
 * as they do there; "eval_dedup", "fused_search", "search_graph" and the kernel switches never change a result.  selected[i] is
 * az_tree_get_selected's value for that tree (-1 unless the move was a Gumbel move).  root_q[i] and root_prior[i] are the root value R and
 * the root's stored priors by action of that same finished tree, by the rule "selfplay_record_search" records them with (az_engine.h,
 * az_selfplay_get_search).
 * So a result depends on nothing but (state, game id, seed, the parameters, the options, the model): not on `concurrent`, not on the order
 * of the positions when their game_ids travel with them, not on which positions shared a chunk, not on states versus boards, not on the
 * state of the evaluation cache.
 *
 * The window is walked in chunks of `concurrent` trees over one pooled tree arena, which later calls of the same shape re-use
 * (az_stats.tree_arena_allocs does not grow).  The window and the outputs are staged once; the host waits for the device twice per call,
 * once for the position check's verdict and once at the end.
 *
 * Every pointer may be host or device memory.  Every output but pi may be NULL.  n = 0 is AZ_OK and runs nothing.
 *
 * Refused with AZ_ERR_BAD_ARGUMENT before any search, the outputs unwritten:
 *   on entry     n < 0 or n > 2^24; a NULL params or pi; states and boards both NULL; num_sims < 1; num_sim_threads outside 0 .. 8 or not
 *                a divisor of num_sims; "gumbel_m" or "forced_playouts_k_e6" together with num_sim_threads > 1; reserve < 8; max_depth < 0;
 *                concurrent < 0; concurrent x num_sim_threads above az_config.max_batch for a conv model; an engine of the second game
 *                (the position check is Connect Four's); an open self-play session (below)
 *   a position   (one check kernel over the whole window; az_last_error names the FIRST offending index)  a feature that is not 0 or 1 or
 *                a cell set in both planes; overlapping stones or bits outside the 7 x 6 board; a stone above an empty cell; stone
 *                counts other than theirs - mine in {0, 1}; a position already decided or full
 * AZ_ERR_NO_MODEL: an id that is not initialised.  AZ_ERR_CAPACITY: a tree ran full (reserve too small); az_last_error names a position
 * and the outputs are unspecified.
 *
 * SESSION CONTRACT (az_engine.h, next to az_selfplay_begin): az_reanalyse runs a tree search, so it is REFUSED while a self-play session
 * is open -- on entry, with an az_last_error that names it, the session's remaining chunks unchanged.  It touches no model's tag or
 * generation, no option, none of the arena's or self-play's logs and no open training session.
 *
 * Stats: moves grows by n; simulations, expansions, link_hits, terminal_hits and leaf_rows_requested by the sum of the n single calls'
 * values; leaf_rows_executed may be smaller (the evaluation cache and the election table work across the trees of a chunk). */
#ifndef AZ_REANALYSE_H
#define AZ_REANALYSE_H

#include "az_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct az_reanalyse_params {
    int32_t concurrent;       /* trees resident at once; 0 = min(n, 8192), for a conv model at most az_config.max_batch / num_sim_threads */
    int32_t num_sims, max_depth, cpuct, model_id;
    int32_t num_sim_threads;  /* 0 = 1, as az_selfplay_params */
    float   temp;             /* of the returned pi, as az_tree_get_action_prob's */
    uint64_t reserve, seed, first_game_id;
} az_reanalyse_params;

az_status az_reanalyse(az_engine* e, const az_reanalyse_params* p, int64_t n,
                       const uint64_t* states /* [n,2] or NULL */, const float* boards /* [n,2,6,7], read when states is NULL */,
                       const uint64_t* game_ids /* [n]; NULL: first_game_id + i */,
                       float* pi /* [n,7] */, float* root_q /* [n] */, float* root_prior /* [n,7] */,
                       uint16_t* counts /* [n,7] */, float* q /* [n,7] */, int32_t* selected /* [n] */);

#ifdef __cplusplus
}
#endif
#endif /* AZ_REANALYSE_H */
