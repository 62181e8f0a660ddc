"""Pure-Python twin of az_rating_fit (alphazero-rs_amd/csrc/az_rating.h): the same operations in the same order on Python floats (IEEE
doubles), so only log10 and sqrt can differ from the library.  TEST INFRASTRUCTURE ONLY."""
import math

MAX_SWEEPS, TOL = 100000, 1e-13


def rating_fit(wld, prior_games=2.0):
    """wld [K][K][3] of ints.  Returns (elo [K], elo_se [K], sweeps, gamma [K])."""
    K = len(wld)
    n = [[0.0] * K for _ in range(K)]
    S = [0.0] * K
    for i in range(K):
        for j in range(K):
            if i == j:
                continue
            W, L, D = (float(int(x)) for x in wld[i][j])
            s = W + D / 2.0 + prior_games / 2.0
            n[i][j] = W + L + D + prior_games
            S[i] += s
    g = [1.0] * K
    sweeps = 0
    for it in range(MAX_SWEEPS):
        g2, total = [0.0] * K, 0.0
        for i in range(K):
            den = 0.0
            for j in range(K):
                if j != i:
                    den += n[i][j] / (g[i] + g[j])
            g2[i] = S[i] / den
            total += g2[i]
        scale = float(K) / total
        delta = 0.0
        for i in range(K):
            g2[i] = g2[i] * scale
            d = abs(g2[i] - g[i]) / g[i]
            if d > delta:
                delta = d
        g = g2
        sweeps = it + 1
        if delta < TOL:
            break
    elo = [400.0 * math.log10(x) for x in g]
    mean = 0.0
    for x in elo:
        mean += x
    mean /= float(K)
    elo = [x - mean for x in elo]
    unit = 400.0 / math.log(10.0)
    se = []
    for i in range(K):
        info = 0.0
        for j in range(K):
            if j != i:
                info += n[i][j] * g[i] * g[j] / ((g[i] + g[j]) * (g[i] + g[j]))
        se.append(unit / math.sqrt(info))
    return elo, se, sweeps, g
