// examples/connect_four.rs (src lines 45-80) on the C++ host: the same Coach::setup parameters, the engine behind it.
// Build:  g++ -std=c++17 -O2 -I include examples/connect_four.cpp -o connect_four -L alphazero-rs_amd -laz_engine
//         (and -Wl,-rpath,$PWD/alphazero-rs_amd)
// Run:    ./connect_four ./checkpoint [num_iters] [num_eps] [num_sims] [num_arena_games] [selfplay_fp8] [root_noise_eps] [root_noise_alpha] [eval_mirror] [playout_cap] [forced_playouts] [arena_openings] [merge_positions] [move_quality] [--gumbel M[,CVISIT,CSCALE]] [--value-target-q L] [--surprise S] [--validation SHARE[,PATIENCE[,best]]] [--reanalyse SIMS] [--search-stop]
//         selfplay_fp8 = 1: the episodes are played in the fp8 class, the arena gate in bf16 (Coach::selfplay_class)
//         root_noise_eps > 0 (e.g. 0.25, with root_noise_alpha 0.3; default alpha 1): Dirichlet root noise in the episodes (Coach::root_noise_eps)
//         eval_mirror = 1: mirror-canonical leaf evaluation for the whole loop, episodes and gate (Coach::eval_mirror)
//         playout_cap = N,P (e.g. 20,0.25): playout cap randomization in the episodes -- a share P of the moves gets the full num_sims and is
//         recorded, every other move gets N simulations and is only played (Coach::playout_cap_sims / playout_cap_full)
//         forced_playouts = K or K,prune (e.g. 2,prune): forced playouts at the root of the episodes' (full) moves, with policy target pruning
//         of the recorded pi (Coach::forced_playouts_k / policy_prune)
//         arena_openings = N (even, 2 .. 12, e.g. 6): paired openings in the gate -- arena game g and its seat-swapped twin start from the same
//         N random quiet plies, every pair from others (Coach::arena_opening_plies)
//         merge_positions = 1, canonical, weighted or canonical,weighted: position averaging before training -- one tuple per distinct position of the window with the mean
//         pi and the mean z of its copies; canonical also merges a position with its mirror image (Coach::merge_positions / merge_canonical); weighted
//         keeps the multiplicities and draws every training row in proportion to them, mirrored at random under canonical (Coach::merge_weighted)
//         move_quality = STONES[,NODES] (e.g. 26): after every arena its games are replayed, the positions with at least STONES stones solved
//         exactly (budget NODES per position and action, default 2^20) and each model's value-losing moves counted (Coach::solve_min_stones)
//         --gumbel M[,CVISIT,CSCALE] (anywhere on the line, e.g. --gumbel 4 or --gumbel 4,50,1): Gumbel root search with sequential halving in
//         the episodes -- at most M root actions considered, the improved policy recorded, the winner played (Coach::gumbel_m / gumbel_c_visit /
//         gumbel_c_scale); not together with forced_playouts
//         --value-target-q L (anywhere on the line, e.g. 0.5): the value target is (1 - L) z + L q, the game outcome mixed with the root value of
//         the tuple's own search (Coach::value_target_q)
//         --surprise S (anywhere on the line, e.g. 0.5): policy surprise weighting -- the iteration's tuples are resampled, a share S of the
//         weight in proportion to KL(pi || root prior) (Coach::surprise_share)
//         --validation SHARE[,PATIENCE[,best]] (anywhere on the line, e.g. 0.05 or 0.05,3,best): held-out validation -- a share SHARE of the
//         window's positions is never trained on and scored at the end of every epoch; PATIENCE > 0 stops after that many epochs without a
//         new best, best keeps the best epoch's weights (Coach::validation_share / patience / keep_best)
//         --reanalyse SIMS (anywhere on the line, e.g. 50): every iteration the pi of every tuple of the older history windows is replaced by a
//         fresh search of SIMS simulations with the current net, before the window is saved and trained on (Coach::reanalyse_sims)
//         --search-stop (anywhere on the line): the decided-move stop for the whole loop -- a temperature-0 search of the episodes and every
//         search of the gate ends once its move can no longer change (Coach::search_stop; include/az_search_stop.h)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "az_host.hpp"

int main(int argc, char** argv) {
    using namespace az_host;
    // take "--name VALUE" out of the line: the positionals keep their places
    auto take = [&](const char* name) {
        std::string v;
        for (int i = 1; i + 1 < argc; ++i) {
            if (std::strcmp(argv[i], name) != 0) continue;
            v = argv[i + 1];
            for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
        return v;
    };
    // ... and the switch "--search-stop", which has no value
    bool search_stop = false;
    for (int i = 1; i < argc; ++i) {
        if (std::strcmp(argv[i], "--search-stop") != 0) continue;
        search_stop = true;
        for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
        argc -= 1;
        break;
    }
    const std::string gumbel = take("--gumbel"), value_q = take("--value-target-q"), surprise_s = take("--surprise"), validation = take("--validation"),
                      reanalyse_s = take("--reanalyse");
    const std::string dir = argc > 1 ? argv[1] : "./checkpoint";
    const size_t iters = argc > 2 ? std::strtoul(argv[2], nullptr, 10) : 1;       // num_iters, examples/connect_four.rs:65
    const size_t eps = argc > 3 ? std::strtoul(argv[3], nullptr, 10) : 1;         // num_eps, :66
    const size_t sims = argc > 4 ? std::strtoul(argv[4], nullptr, 10) : 25;       // num_sims, :67
    const size_t arena = argc > 5 ? std::strtoul(argv[5], nullptr, 10) : 40;      // num_arena_games, :64
    const bool selfplay_fp8 = argc > 6 && std::strtoul(argv[6], nullptr, 10) != 0;
    const double noise_eps = argc > 7 ? std::atof(argv[7]) : 0.0, noise_alpha = argc > 8 ? std::atof(argv[8]) : 1.0;
    const bool eval_mirror = argc > 9 && std::strtoul(argv[9], nullptr, 10) != 0;
    const std::string cap = argc > 10 ? argv[10] : "";
    const size_t comma = cap.find(',');
    const long cap_sims = cap.empty() ? 0 : std::strtol(cap.c_str(), nullptr, 10);
    const double cap_full = comma == std::string::npos ? 0.25 : std::atof(cap.c_str() + comma + 1);
    const std::string forced = argc > 11 ? argv[11] : "";
    const double forced_k = forced.empty() ? 0.0 : std::atof(forced.c_str());
    const bool prune = forced.find(",prune") != std::string::npos;
    const long arena_openings = argc > 12 ? std::strtol(argv[12], nullptr, 10) : 0;
    const std::string merge = argc > 13 ? argv[13] : "0";
    const std::string quality = argc > 14 ? argv[14] : "0";
    try {
        Engine e(0, 8192, 512);
        if (az_net_load(e.raw(), 0, (dir + "/0.aznet").c_str()) != AZ_OK) e.check(az_net_init_random(e.raw(), 0, 0));
        Coach coach = Coach::setup(e, dir, 1000000, 0.6f, 15, 20, 200000, 1, /*concurrent game slots*/ 8192, arena, iters, eps, sims, 1,
                                   1000, 1);
        if (selfplay_fp8) coach.selfplay_class = AZ_NET_CLASS_FP8;
        coach.eval_mirror = eval_mirror;
        coach.root_noise_eps = noise_eps; coach.root_noise_alpha = noise_alpha;
        coach.playout_cap_sims = cap_sims; coach.playout_cap_full = cap_full;
        coach.forced_playouts_k = forced_k; coach.policy_prune = prune;
        if (!value_q.empty()) coach.value_target_q = std::atof(value_q.c_str());
        if (!surprise_s.empty()) coach.surprise_share = std::atof(surprise_s.c_str());
        if (!validation.empty()) {
            coach.validation_share = std::atof(validation.c_str());
            const size_t c1 = validation.find(','), c2 = c1 == std::string::npos ? c1 : validation.find(',', c1 + 1);
            if (c1 != std::string::npos) coach.patience = (size_t)std::strtoul(validation.c_str() + c1 + 1, nullptr, 10);
            coach.keep_best = c2 != std::string::npos && validation.substr(c2 + 1) == "best";
        }
        coach.search_stop = search_stop;
        if (!reanalyse_s.empty()) coach.reanalyse_sims = (size_t)std::strtoul(reanalyse_s.c_str(), nullptr, 10);
        if (!gumbel.empty()) {
            coach.gumbel_m = std::strtol(gumbel.c_str(), nullptr, 10);
            const size_t c1 = gumbel.find(','), c2 = c1 == std::string::npos ? c1 : gumbel.find(',', c1 + 1);
            if (c1 != std::string::npos) coach.gumbel_c_visit = std::atof(gumbel.c_str() + c1 + 1);
            if (c2 != std::string::npos) coach.gumbel_c_scale = std::atof(gumbel.c_str() + c2 + 1);
        }
        coach.arena_opening_plies = arena_openings;
        coach.merge_canonical = merge == "canonical" || merge == "canonical,weighted";
        coach.merge_weighted = merge == "weighted" || merge == "canonical,weighted";
        coach.merge_positions = coach.merge_canonical || coach.merge_weighted || std::strtol(merge.c_str(), nullptr, 10) != 0;
        coach.solve_min_stones = (size_t)std::strtoul(quality.c_str(), nullptr, 10);
        if (quality.find(',') != std::string::npos) coach.solve_max_nodes = (uint32_t)std::strtoul(quality.c_str() + quality.find(',') + 1, nullptr, 10);
        for (const auto& r : coach.learn(false, /*seed*/ 0)) {
            std::printf("iteration %zu: %zu samples, new/prev/draw %zu/%zu/%zu, %s, loss (%.4f, %.4f)\n", r.iteration, r.samples, r.nwins,
                        r.pwins, r.draws, r.accepted ? "accepted" : "rejected", r.losses.empty() ? 0.f : r.losses[r.losses.size() - 2],
                        r.losses.empty() ? 0.f : r.losses.back());
            if (coach.merge_positions) std::printf("iteration %zu: merged from %zu raw samples\n", r.iteration, r.samples_raw);
            if (coach.validation_share > 0 && !r.val_loss_pi.empty())
                std::printf("iteration %zu: %zu held out, %zu epochs, best epoch %d with val loss (%.4f, %.4f) top1 %.4f\n", r.iteration, r.val_n, r.val_loss_pi.size(),
                            (int)r.best_epoch, r.val_loss_pi[(size_t)r.best_epoch], r.val_loss_v[(size_t)r.best_epoch], r.val_top1[(size_t)r.best_epoch]);
            if (coach.reanalyse_sims > 0) std::printf("iteration %zu: %zu older tuples re-searched in %.2f s\n", r.iteration, r.reanalysed, r.t_reanalyse);
            if (coach.merge_weighted) std::printf("iteration %zu: rows drawn by multiplicity, total weight %zu\n", r.iteration, r.samples_weight);
        }
        return 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "panic: %s\n", ex.what());
        return 1;
    }
}
