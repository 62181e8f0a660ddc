"""Layer-by-layer reference of the bf16 inference net in float64 on the CPU, with the error bounds the layer tests hold the
kernels to (tests/test_net_layers_cpu.py, tests/test_net_layers_gpu.py).

Layouts are the engine's: activations channels-last ([n][h][w][C]), K index of a conv = tap * C + ci with tap = ky * 3 + kx, fc1's
input index = (y * 3 + x) * C + c of conv4's [2][3][C] output, board row y counted from the top, bit of cell (y, x) = x * 7 + (5 - y).

Two bounds, both derived (nothing here is a measurement):

  exact data   integer-valued parameters and BatchNorm folding to exactly 1 (net_ref.exact_params): every product and partial sum is
               an integer; while S = sum |a||w| + |b| < 2^24 every f32 summation order is exact, so the stored bf16 (f16 for the
               conv2 table) must be the round-to-nearest-even of the exact sum, bit for bit.
  random data  |dev - y| <= 2^-8 |y| + (K + 1) 2^-23 S per element: bf16's worst half ulp plus the worst case of any f32 summation
               order of K products and a bias with truncating partial sums.  For an f16 table entry 2^-11 |u| + 2^-25 (f16's half
               ulp, and half of the subnormal spacing 2^-24) takes the place of the first term.
"""
import numpy as np
import torch

from net_ref import unpack

BN_EPS = np.float32(1e-3)
PATTERNS = 19683
LAYERS = ("conv2", "conv3", "conv4", "fc1", "fc2")
POW3 = 3 ** np.arange(9)


def layer_k(name, C):
    """Number of products per output element of a GEMM layer (the K of the random-data bound; + 1 for the bias)."""
    return {"conv2": 9 * C, "conv3": 9 * C, "conv4": 9 * C, "fc1": 6 * C, "fc2": 1024}[name]


# ---- number formats -------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float array -> the uint16 bit patterns of its round-to-nearest-even bf16 values."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(torch.float32).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16)


def bf16_from_bits(u):
    """uint16 bf16 bit patterns -> float64 values."""
    u = np.ascontiguousarray(u, dtype=np.uint16)
    return (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_round64(x):
    return bf16_from_bits(bf16_bits(x))


def f16_bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).astype(np.float16).view(np.uint16)


def f16_from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint16).view(np.float16).astype(np.float64)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def arbitrary_states(n, seed):
    """n canonical (mine, theirs) bitboards with every one of the 42 cells independently empty / mine / theirs: not legal positions
    (stones float), so every position carries a uniformly random conv1 pattern -- random play only ever produces ~4000 of the 19683."""
    g = np.random.default_rng(seed)
    cell = g.integers(0, 3, (n, 6, 7))
    out = np.zeros((n, 2), np.uint64)
    for y in range(6):
        for x in range(7):
            bit = np.uint64(1 << (x * 7 + (5 - y)))
            out[:, 0] |= np.where(cell[:, y, x] == 1, bit, np.uint64(0))
            out[:, 1] |= np.where(cell[:, y, x] == 2, bit, np.uint64(0))
    return out


def cells_of(states):
    """[n][6][7] int: 0 empty, 1 mine, 2 theirs (row 0 = top)."""
    s = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 2)
    cell = np.zeros((s.shape[0], 6, 7), np.int64)
    for y in range(6):
        for x in range(7):
            sh = np.uint64(x * 7 + (5 - y))
            mine = ((s[:, 0] >> sh) & np.uint64(1)).astype(np.int64)
            theirs = ((s[:, 1] >> sh) & np.uint64(1)).astype(np.int64)
            cell[:, y, x] = np.where(mine == 1, 1, np.where(theirs == 1, 2, 0))
    return cell


def boards_of(states):
    """to_features: [n][2][6][7] f32 planes (mine, theirs)."""
    cell = cells_of(states)
    return np.stack([(cell == 1), (cell == 2)], axis=1).astype(np.float32)


def patterns_of(states):
    """conv1_pattern of every position: [n][6][7] int, sum over taps t = ky * 3 + kx of cell(y + ky - 1, x + kx - 1) * 3^t, a cell
    outside the board counting as empty."""
    cell = cells_of(states)
    pad = np.zeros((cell.shape[0], 8, 9), np.int64)
    pad[:, 1:7, 1:8] = cell
    pat = np.zeros_like(cell)
    for t in range(9):
        ky, kx = divmod(t, 3)
        pat += pad[:, ky:ky + 6, kx:kx + 7] * POW3[t]
    return pat


# ---- the fold -------------------------------------------------------------------------------------------------------
def _bf16_f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def fold_like_engine(params, C):
    """The f32 fold of the engine's weight upload: s = gamma / sqrt(var + 1e-3f), w * s, b * s + (beta - mean * s), every operation in
    f32; the weights of conv2 .. fc2 rounded to bf16 (nearest even), conv1 and the heads left in f32.
    -> {"conv1": (w [18][C], b [C]), "conv2".."fc2": (w [K][N], b [N]), "pi": (w [512][7], b [7]), "v": (w [512], b)} as float32."""
    P = {k: v.numpy() for k, v in unpack(np.asarray(params, np.float32), C).items()}
    out = {}
    for name in ("conv1",) + LAYERS:
        w, b, bn = P[name + "_w"], P[name + "_b"], P[name + "_bn"]
        n_out = w.shape[-1]
        w = w.reshape(-1, n_out)
        s = (bn[0] / np.sqrt(bn[3] + BN_EPS)).astype(np.float32)
        wf = (w * s).astype(np.float32)
        bf = (b * s + (bn[1] - bn[2] * s)).astype(np.float32)
        assert wf.dtype == np.float32 and bf.dtype == np.float32
        out[name] = (wf if name == "conv1" else _bf16_f32(wf), bf)
    out["pi"] = (P["pi_w"], P["pi_b"])
    out["v"] = (P["v_w"].reshape(512), P["v_b"].reshape(()))
    return out


# ---- layers ---------------------------------------------------------------------------------------------------------
def _gemm_form(name, a_in, w, dtype):
    """sum a * w of a GEMM layer in `dtype`, tap by tap: conv2 is 'same' (zero halo), conv3 / conv4 are 'valid', the FCs one tap."""
    a = torch.from_numpy(np.ascontiguousarray(a_in)).to(dtype)
    w = torch.from_numpy(np.ascontiguousarray(w)).to(dtype)
    if name in ("fc1", "fc2"):
        return a.reshape(a.shape[0], -1) @ w
    n, h, wd, C = a.shape
    if name == "conv2":
        pad = torch.zeros((n, h + 2, wd + 2, C), dtype=dtype)
        pad[:, 1:-1, 1:-1] = a
        a, h, wd = pad, h + 2, wd + 2
    oh, ow = h - 2, wd - 2
    acc = torch.zeros((n * oh * ow, w.shape[1]), dtype=dtype)
    for t in range(9):
        ky, kx = divmod(t, 3)
        acc += a[:, ky:ky + oh, kx:kx + ow, :].reshape(-1, C) @ w[t * C:(t + 1) * C]
    return acc.reshape(n, oh, ow, -1)


def layer_ref(name, a_in, folded, dtype=torch.float64):
    """One GEMM layer (name in LAYERS) from ITS OWN input activations (float64 copies of bf16 values; conv: [n][h][w][C], fc: [n][K] or
    anything that flattens to it) -> (y, S) in float64: y = relu(sum a w + b) unrounded, S = sum |a||w| + |b|.
    dtype = torch.float32 computes the same sums in f32: exact, and equal to float64, whenever every term is an integer and S < 2^24."""
    w, b = folded[name]
    y = _gemm_form(name, a_in, w, dtype).to(torch.float64).numpy() + b.astype(np.float64)
    S = _gemm_form(name, np.abs(a_in), np.abs(w), dtype).to(torch.float64).numpy() + np.abs(b.astype(np.float64))
    return np.maximum(y, 0.0), S


def conv1_table_ref(folded):
    """All 19683 rows of conv1's pattern table: (y [19683][C], S) in float64; digit t of the pattern index = tap t = ky * 3 + kx,
    0 empty / outside, 1 mine, 2 theirs."""
    w, b = folded["conv1"]
    w = w.astype(np.float64).reshape(9, 2, -1)
    q = np.arange(PATTERNS)
    y = np.tile(b.astype(np.float64), (PATTERNS, 1))
    S = np.abs(y)
    for t in range(9):
        d = (q // POW3[t]) % 3
        for ci in range(2):
            sel = (d == ci + 1)[:, None]
            y = y + sel * w[t, ci]
            S = S + sel * np.abs(w[t, ci])
    return np.maximum(y, 0.0), S


def conv1_ref(states, folded):
    """conv1 of boards computed directly (no table): (y [n][6][7][C], S)."""
    w, b = folded["conv1"]
    w = w.astype(np.float64).reshape(9, 2, -1)
    cell = cells_of(states)
    pad = np.zeros((cell.shape[0], 8, 9), np.int64)
    pad[:, 1:7, 1:8] = cell
    y = np.zeros(cell.shape + (w.shape[-1],)) + b.astype(np.float64)
    S = np.abs(y)
    for t in range(9):
        ky, kx = divmod(t, 3)
        nb = pad[:, ky:ky + 6, kx:kx + 7]
        for ci in range(2):
            sel = (nb == ci + 1)[..., None]
            y = y + sel * w[t, ci]
            S = S + sel * np.abs(w[t, ci])
    return np.maximum(y, 0.0), S


def u_ref(T, folded, dtype=torch.float64):
    """conv2's table from conv1 table rows T [rows][C] (float64 copies of bf16 values): U[q][t][co] = sum_ci W2[co][t][ci] T[q][ci]
    (no bias, no ReLU) -> (U [rows][9][C], S) in float64."""
    w = folded["conv2"][0]
    C = w.shape[1]
    wt = torch.from_numpy(np.ascontiguousarray(w.reshape(9, C, C).transpose(1, 0, 2).reshape(C, 9 * C))).to(dtype)   # [ci][t * C + co]
    t = torch.from_numpy(np.ascontiguousarray(T)).to(dtype)
    U = (t @ wt).to(torch.float64).numpy().reshape(-1, 9, C)
    S = (t.abs() @ wt.abs()).to(torch.float64).numpy().reshape(-1, 9, C)
    return U, S


def table_conv2_ref(U_of, states, folded):
    """conv2 as the table gather: relu(b + the in-board taps of U[pattern of the neighbour][t]) -> (y [n][6][7][C], S).
    U_of(patterns) returns the float64 table rows [len(patterns)][9][C] for an int array of pattern indices."""
    b = folded["conv2"][1].astype(np.float64)
    pat = patterns_of(states)
    n = pat.shape[0]
    uniq, inv = np.unique(pat, return_inverse=True)
    rows = U_of(uniq)                                          # [u][9][C]
    inv = inv.reshape(n, 6, 7)
    C = rows.shape[-1]
    y = np.zeros((n, 6, 7, C)) + b
    S = np.abs(y)
    for t in range(9):
        ky, kx = divmod(t, 3)
        y0, y1, x0, x1 = max(0, 1 - ky), min(6, 7 - ky), max(0, 1 - kx), min(7, 8 - kx)      # outputs whose neighbour is on the board
        g = rows[inv[:, y0 + ky - 1:y1 + ky - 1, x0 + kx - 1:x1 + kx - 1], t]
        y[:, y0:y1, x0:x1] += g
        S[:, y0:y1, x0:x1] += np.abs(g)
    return np.maximum(y, 0.0), S


def heads_ref(fc2o, folded):
    """The heads in float64 from fc2's output -> (pi [n][7], v [n], logit bound [n]): the last is 513 * 2^-23 * S, the largest of a
    row's eight logits' bounds (any f32 order of 512 products and a bias)."""
    x = np.asarray(fc2o, np.float64)
    pw, pb = (a.astype(np.float64) for a in folded["pi"])
    vw, vb = (a.astype(np.float64) for a in folded["v"])
    lp, lv = x @ pw + pb, x @ vw + vb
    S = np.maximum((np.abs(x) @ np.abs(pw) + np.abs(pb)).max(axis=1), np.abs(x) @ np.abs(vw) + np.abs(vb))
    e = np.exp(lp - lp.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True), np.tanh(lv), 513 * 2.0 ** -23 * S


# ---- bounds ---------------------------------------------------------------------------------------------------------
def bound_bf16(y, S, K):
    """The random-data bound of a bf16 output that sums K products and a bias in f32."""
    return 2.0 ** -8 * np.abs(y) + (K + 1) * 2.0 ** -23 * S


def bound_f16(u, S, K):
    """... of an f16 conv2-table entry that sums K products (no bias)."""
    return 2.0 ** -11 * np.abs(u) + 2.0 ** -25 + K * 2.0 ** -23 * S


def worst_ratio(dev, y, bound):
    """max over ALL elements of |dev - y| / bound (a zero bound with a zero error counts as 0, with any error as inf)."""
    assert np.shape(dev) == np.shape(y) == np.shape(bound), (np.shape(dev), np.shape(y), np.shape(bound))     # no broadcasting: every element
    err = np.abs(np.asarray(dev, np.float64) - y)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.nan_to_num(r, nan=np.inf).max())


# ---- the whole exact forward ----------------------------------------------------------------------------------------
def conv1_rows(states, T):
    """conv1's output [n][6][7][C] as rows of a pattern table T [19683][C]."""
    return T[patterns_of(states)]


def conv1_from_table(states, table_ref):
    """conv1_ref's (y, max S) from conv1_table_ref's (T, S): the rows of the states' patterns.  For thousands of states the 19683-row
    table, computed once, is several times cheaper than conv1_ref on every board; the two are the same sums of the same terms."""
    T, S = table_ref
    pat = patterns_of(states)
    return T[pat], float(S[np.unique(pat)].max())


def forward_layers(states, folded, dtype=torch.float64, table=None, conv1=None):
    """The net layer by layer, each layer from the bf16 rounding of the one before (what the device stores):
    -> {"t1": conv1 rows, "conv2" .. "fc2": (y unrounded, S, stored = bf16-rounded y as float64), "S1": max S of conv1}.
    table = a U_of callable (table_conv2_ref) computes conv2 from the conv2 table instead of the GEMM form.
    conv1 = conv1_from_table's pair takes the place of conv1_ref on every board."""
    y1, S1 = conv1_ref(states, folded) if conv1 is None else conv1
    out = {"t1": bf16_round64(y1), "S1": float(np.max(S1))}
    a = out["t1"]
    for name in LAYERS:
        if name == "conv2" and table is not None:
            y, S = table_conv2_ref(table, states, folded)
        else:
            y, S = layer_ref(name, a, folded, dtype)
        a = bf16_round64(y)
        out[name] = (y, S, a)
    return out


# ---- what the CPU and the GPU tests share: parameters and inputs ------------------------------------------------------
EXACT_SEED = 5
HEAD_SHIFT = {128: 18, 256: 18, 384: 20, 512: 21}     # exact_params' head weights 2^-shift: logits O(1) at every width (asserted, CPU test)
N_LEGAL = N_ARBITRARY = 75


def u2_rows(C):
    """The conv2-table rows the tests read: all 19684 up to C = 256; above, every 16th plus everything from 19456 on (the table
    GEMM's last two 128-row tiles, the second ragged: 19683 = 153 * 128 + 99, and the appended zero row)."""
    if C <= 256:
        return np.arange(PATTERNS + 1)
    return np.unique(np.concatenate([np.arange(0, PATTERNS + 1, 16), np.arange(19456, PATTERNS + 1)]))


def layer_states(random_states, oracle):
    """The inputs of the layer tests: 75 positions of random legal play (test_net_gpu.random_states) + 75 arbitrary boards."""
    return np.concatenate([random_states(oracle, N_LEGAL, seed=21).reshape(-1, 2), arbitrary_states(N_ARBITRARY, seed=22)])


def exact_conditions(out, pi, v):
    """The conditions under which exact data demand bit-for-bit results, from the reference alone (out = forward_layers, pi / v =
    heads_ref of its fc2): raises AssertionError naming the condition that fails."""
    assert out["S1"] < 2 ** 24
    assert np.unique(out["t1"]).size > 2 and (out["t1"] != 0).mean() > 0.1
    for name in LAYERS:
        y, S, stored = out[name]
        assert S.max() < 2 ** 24, (name, S.max())                               # every f32 order is exact
        assert np.array_equal(y, np.rint(y)), name                              # ... of integers
        assert np.unique(stored).size > 16 and (stored != 0).mean() > 0.1, name  # the layer is alive
    assert pi.max() < 0.999 and np.abs(v).max() < 0.999                         # nothing saturated that could hide a difference
