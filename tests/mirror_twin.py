"""Plain-Python restatement of the "eval_mirror" contract (include/az_engine.h): the canonical state c(s) and "F from N".
Nothing here is shared with the engine: python ints and numpy only.

Bitboards: bit(col, row) = col * 7 + row, row 0 = bottom; a state is (mine, theirs), `mine` = the side to move."""
import numpy as np

BOTTOM = sum(1 << (7 * c) for c in range(7))


def mirror_bits(b):
    b = int(b)
    return sum(((b >> (7 * c)) & 0x7F) << (7 * (6 - c)) for c in range(7))


def pack(mine, theirs):
    """Game::pack: one bit above every column's stones plus the mover's stones below it."""
    mine, theirs = int(mine), int(theirs)
    return mine + (mine | theirs) + BOTTOM


def mirror(s):
    return mirror_bits(s[0]), mirror_bits(s[1])


def canonical(s):
    """c(s) and the flag: s or mirror(s), whichever packs to the smaller word; on equal words s itself, not mirrored."""
    s = (int(s[0]), int(s[1]))
    m = mirror(s)
    return (m, 1) if pack(*m) < pack(*s) else (s, 0)


def _mirror_bits_np(b):
    b = np.asarray(b, np.uint64)
    r = np.zeros_like(b)
    for c in range(7):
        r |= ((b >> np.uint64(7 * c)) & np.uint64(0x7F)) << np.uint64(7 * (6 - c))
    return r


def pack_batch(states):
    s = np.asarray(states, np.uint64).reshape(-1, 2)
    return s[:, 0] + (s[:, 0] | s[:, 1]) + np.uint64(BOTTOM)


def mirror_batch(states):
    s = np.asarray(states, np.uint64).reshape(-1, 2)
    return np.stack([_mirror_bits_np(s[:, 0]), _mirror_bits_np(s[:, 1])], axis=1)


def canonical_batch(states):
    """states [n, 2] uint64 -> (canonical states [n, 2] uint64, flags [n] uint8): canonical() on whole arrays"""
    s = np.asarray(states, np.uint64).reshape(-1, 2)
    m = mirror_batch(s)
    flags = pack_batch(m) < pack_batch(s)
    return np.where(flags[:, None], m, s), flags.astype(np.uint8)


def f_from_n(predict, states):
    """F(s): canonicalise, call predict(states [n, 2] uint64) -> (pi [n, 7], v [n]) of the raw net N, un-mirror pi."""
    c, flags = canonical_batch(states)
    pi, v = predict(c)
    pi = np.array(pi, np.float32).reshape(-1, 7)
    m = flags.astype(bool)
    pi[m] = pi[m][:, ::-1]
    return pi, np.array(v, np.float32).reshape(-1)


_SHIFT = np.array([[c * 7 + (5 - r) for c in range(7)] for r in range(6)], np.uint64)      # plane row r (0 = top), column c


def boards_to_states(boards):
    """[n, 2, 6, 7] 0/1 planes (row 0 = top) -> [n, 2] uint64"""
    b = (np.asarray(boards).reshape(-1, 2, 6, 7) != 0).astype(np.uint64)
    return (b << _SHIFT).sum(axis=(2, 3), dtype=np.uint64)


def states_to_boards(states):
    s = np.asarray(states, np.uint64).reshape(-1, 2)
    return ((s[:, :, None, None] >> _SHIFT) & np.uint64(1)).astype(np.float32)
