"""Repeat-rich texts for the tie route of the hybrid initial sort, and a witness of what that route is expected to do.

The hybrid initial sort (sfx_radix.hip, hybrid_sort_e64_text) takes texts of 2^25 .. 2^28 suffixes with keys of >= 24 bits.
Without an oversized sub-bucket its LDS sort leaves one tie bit per slot; k_tie_direct orders the short stretches of tied slots
in place and everything else goes through k_tie_heads, k_tie_list, the small-groups pass and refine (sfx_sa.hip).  Uniform
random text never reaches that leftover path at these sizes; the generators below plant the repeats that do, and `witness`
predicts, from the text and the oracle's SA and LCP alone (never from the engine), which stretches the route leaves over.

Everything is deterministic: numpy generators with fixed seeds on top of _gen.dna / _gen.uniform_bytes.
"""
import numpy as np

import _gen

LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
RUN_MAX = 8                     # kTieRunMax: the longest stretch k_tie_direct orders in place
SUB_CAP = 16384                 # kBucketNW * kWave * kBucketKPT: the largest sub-bucket the LDS sort holds
SLOW = 4096                     # sub-buckets above this count against the route's 1/64 tolerance
DEPTH_WORDS = 16                # kSmallDepthWords: k_tie_direct compares kSmallDepthWords / 2 pairs of packed 32-bit words
M_PLANTED = (1 << 25) + 4099    # (the last word of the tie mask is partial)
H_DOUBLED = (1 << 24) + 2049
M_SMALL = 1 << 25
M_BIG = 240_000_003             # ~0.9 x 2^28: most waves of k_tie_direct take two passes of its grid-stride loop (2^28 of DNA would
                                # put half the text in sub-buckets above 4096: the four-pass sort)


def _place(m, pieces, rng, tail=0):
    """Random non-overlapping start offsets in [0, m - tail) for `pieces` (uint8 arrays)."""
    lens = np.array([len(p) for p in pieces], dtype=np.int64)
    free = m - tail - int(lens.sum())
    assert free > 0, "the planted pieces do not fit"
    order = rng.permutation(len(pieces))
    gaps = np.sort(rng.integers(0, free + 1, len(pieces)))
    starts = np.empty(len(pieces), dtype=np.int64)
    starts[order] = gaps + np.concatenate(([0], np.cumsum(lens[order])[:-1]))
    return starts


def _plant(text, pieces, rng, tail=0):
    for p, s in zip(pieces, _place(len(text), pieces, rng, tail)):
        text[s:s + len(p)] = p
    return text


def planted_dna(m, seed=0x71E5, slices=False):
    """m symbols of uniform DNA with planted repeats (every copy at its own random place, none overlapping):
      - blocks of 24, 40, 300 and 2000 symbols in c copies for c in {2, 3, 5, 8, 9, 16, 33, 34, 64, 200}, and blocks of 24 and 40
        symbols in 1000 and 3000 copies: stretches of tied slots in every length class, long ones across 64- and 4096-slot
        boundaries, short ones equal beyond k_tie_direct's depth;
      - one 1 MiB segment twice;
      - 240 tandem repeats, a unit of 1 .. 6 symbols (not all A) 50 .. 500 times;
      - a run of 5000 A (the smallest symbol: its code is the zero padding past the end) inside the text and 40 at its end.
    slices=True: the blocks of 24 and 40 symbols and the 40 A at the end only.  A slice of the range-partitioned build has text
    rounds only, and longer repeats (the 300- and 2000-symbol blocks, the segment, the tandem repeats, the run of 5000 A) stall
    them until the slice asks for the whole array (SFX_ERR_NEEDS_RANKS, seen on an MI355X)."""
    rng = np.random.default_rng(seed)
    text = _gen.dna(m, seed=seed).copy()
    pieces = []
    for length in (24, 40) if slices else (24, 40, 300, 2000):
        for c in (2, 3, 5, 8, 9, 16, 33, 34, 64, 200):
            pieces += [LETTERS[rng.integers(0, 4, length)]] * c
    for length in (24, 40):
        for c in (1000, 3000):
            pieces += [LETTERS[rng.integers(0, 4, length)]] * c
    if not slices:
        pieces += [LETTERS[rng.integers(0, 4, 1 << 20)]] * 2
        for _ in range(240):
            unit = LETTERS[rng.integers(0, 4, int(rng.integers(1, 7)))]
            if (unit == ord("A")).all():      # (runs of A have their own piece: at 0.9 x 2^28 more of them would overfill a sub-bucket)
                unit = unit.copy()
                unit[0] = ord("C")
            pieces.append(np.tile(unit, int(rng.integers(50, 501))))
        pieces.append(np.full(5000, ord("A"), dtype=np.uint8))
    _plant(text, pieces, rng, tail=40)
    text[m - 40:] = ord("A")
    return text


def planted_dna_small(m=100_000, seed=0x5E11):
    """planted_dna's shapes at emulator size: blocks of 24, 40 and 300 symbols in 2 .. 64 copies, one 3000-symbol segment twice,
    20 tandem repeats, runs of A inside the text (600) and at its end (40)."""
    rng = np.random.default_rng(seed)
    text = _gen.dna(m, seed=seed).copy()
    pieces = []
    for length in (24, 40, 300):
        for c in (2, 3, 5, 8, 9, 16, 33, 64):
            pieces += [LETTERS[rng.integers(0, 4, length)]] * c
    pieces += [LETTERS[rng.integers(0, 4, 3000)]] * 2
    for _ in range(20):
        pieces.append(np.tile(LETTERS[rng.integers(0, 4, int(rng.integers(2, 7)))], int(rng.integers(20, 200))))
    pieces.append(np.full(600, ord("A"), dtype=np.uint8))
    _plant(text, pieces, rng, tail=40)
    text[m - 40:] = ord("A")
    return text


def doubled_dna(h, seed=0xD0B1E):
    """X + X for X uniform DNA of h symbols: nearly every slot is tied to its partner h positions away."""
    x = _gen.dna(h, seed=seed)
    return np.concatenate([x, x])


def planted_small_alphabet(m, sigma, seed=0x5A11):
    """m symbols uniform over the first `sigma` capital letters (sigma = 2: 32 one-bit symbols per 32-bit key; sigma = 16: 8
    four-bit ones) with planted blocks long enough to tie on the longer key of a text-fed build (33 / 9 symbols), the longest
    of them equal beyond k_tie_direct's depth (512 / 128 symbols), in 2 .. 300 copies."""
    assert sigma in (2, 16)
    rng = np.random.default_rng(seed)
    text = _gen.uniform_bytes(m, sigma, seed, base=65).copy()
    lengths = (48, 80, 700) if sigma == 2 else (16, 40, 200)
    pieces = []
    for length in lengths:
        for c in (2, 3, 5, 8, 9, 16, 33, 64, 300):
            pieces += [(rng.integers(0, sigma, length) + 65).astype(np.uint8)] * c
    return _plant(text, pieces, rng)


def gpu_texts():
    """name -> (generator, size): the texts of tests/test_gpu_tie_route.py of ~2^25 suffixes, at the sizes it builds them."""
    return {
        "planted_dna": (lambda: planted_dna(M_PLANTED), M_PLANTED),
        "doubled_dna": (lambda: doubled_dna(H_DOUBLED), 2 * H_DOUBLED),
        "binary": (lambda: planted_small_alphabet(M_SMALL + 77, 2), M_SMALL + 77),
        "sigma16": (lambda: planted_small_alphabet(M_SMALL + 123, 16), M_SMALL + 123),
    }


# ---- the witness ----------------------------------------------------------------------------------------------------------------

def codes_of(text):
    """(codes, bits, symbols_per_key): a byte's code is its rank among the bytes present, bits = ceil(log2 sigma) (>= 1), and the
    32-bit key holds 32 // bits symbols."""
    t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, dtype=np.uint8)
    present = np.bincount(t, minlength=256) > 0
    rank = (np.cumsum(present) - 1).astype(np.uint8)
    sigma = int(present.sum())
    bits = max(1, (max(sigma, 2) - 1).bit_length())
    return rank[t], bits, 32 // bits


def prefix_keys(codes, bits, nsym):
    """The first `nsym` symbols of every suffix as one integer (uint64), zero-padded past the end: windows of 1, 2, 4, ... symbols
    by doubling, then the key from the windows of nsym's binary digits."""
    n = len(codes)
    assert nsym * bits <= 64
    cur = np.concatenate([codes.astype(np.uint64), np.zeros(nsym, dtype=np.uint64)])
    win, w = {}, 1
    while True:
        if nsym & w:
            win[w] = cur
        if 2 * w > nsym:
            break
        cur = (cur[:len(cur) - w] << np.uint64(w * bits)) | cur[w:]
        w *= 2
    del cur
    key = np.zeros(n, dtype=np.uint64)
    off = 0
    for w in sorted(win, reverse=True):
        if nsym - off >= w:
            key = (key << np.uint64(w * bits)) | win[w][off:off + n]
            off += w
    return key


def route_preconditions(text):
    """The hybrid route's entry test on the sub-bucket histogram (sfx_radix.hip:1903 k_hist16_scan, :1923 `give_way`; tie mode
    needs no oversized sub-bucket): a sub-bucket holds the suffixes that share the top 16 bits of their 32-bit key.  From the text
    alone.  -> dict: largest sub-bucket, suffixes in sub-buckets above 4096, ok = none above 16384 and those at most m / 64."""
    codes, bits, spk = codes_of(text)
    m = len(codes)
    top = 16 // bits
    padded = np.concatenate([codes, np.zeros(top, dtype=np.uint8)])
    hist = np.zeros(1 << 16, dtype=np.int64)
    for a in range(0, m, 1 << 24):
        b = min(m, a + (1 << 24))
        k = np.zeros(b - a, dtype=np.int64)
        for j in range(top):
            k = (k << bits) | padded[a + j:b + j]
        hist += np.bincount(k, minlength=1 << 16)
    largest = int(hist.max())
    slow = int(hist[hist > SLOW].sum())
    return {"m": m, "largest": largest, "slow": slow, "ok": largest <= SUB_CAP and slow * 64 <= m}


def _runs(flag):
    """(starts, lengths) of the maximal runs of True in a bool array."""
    d = np.diff(np.concatenate(([0], flag.astype(np.int8), [0])))
    starts = np.flatnonzero(d == 1)
    return starts, np.flatnonzero(d == -1) - starts


def witness(text, sa, lcp, text_fed=True, key_symbols=None):
    """What the tie route does with `text`, modelled from the oracle's SA and LCP (lcp[r] = LCP of slots r - 1 and r).

    key_symbols: the symbols the initial sort keys on, where the caller knows them (tests/_routes.py: symbols_per_key of the
    ordinary route -- 2 * (32 // bits) on fixed-width 64-bit keys -- and of a hybrid sort whose symbols are wider than 4 bits, one
    more on the hybrid route's tie mode with 1-, 2- or 4-bit symbols); None: from `text_fed`, as below.

    Keys (sfx_radix.hip:1925-1932, SrcText36): a text-fed build sorts on symbols_per_key + 1 symbols (one more symbol in the four
    bits a suffix index of <= 2^28 leaves free); a slice of a multi-range build on symbols_per_key.  Slot r is tied when its key
    equals the key of slot r - 1 or r + 1; a stretch is a maximal run of tied slots (it may hold several runs of equal keys).
    k_tie_direct orders a stretch of at most RUN_MAX slots in place unless two members share D or more symbols (direct_compare64
    with kSmallDepthWords / 2 steps of two packed words: 256 symbols of DNA, 512 binary, 128 at four bits); every other stretch
    is left over.  k_tie_heads cuts the leftover slots into runs of equal 32-bit key, and the driver takes the small-groups pass
    first when small_groups_pay(kept, groups) (sfx_sa.hip:2137, groups * 4 >= kept)."""
    codes, bits, spk = codes_of(text)
    m = len(codes)
    nsym = int(key_symbols) if key_symbols is not None else (spk + 1 if text_fed else spk)
    assert nsym >= spk, (nsym, spk)
    depth = DEPTH_WORDS // 2 * 2 * spk
    sa = np.asarray(sa)
    key = prefix_keys(codes, bits, nsym)[sa]            # (in SA order)
    eq = key[1:] == key[:-1]
    tied = np.zeros(m, dtype=bool)
    tied[1:] |= eq
    tied[:-1] |= eq
    del eq
    starts, lens = _runs(tied)
    ends = starts + lens
    # the deepest pair of a stretch is its deepest neighbouring pair: max LCP over the slots (start, end)
    lcp_pad = np.concatenate([np.asarray(lcp, dtype=np.int64), [0]])
    idx = np.empty(2 * len(starts), dtype=np.int64)
    idx[0::2] = starts + 1
    idx[1::2] = ends
    deepest = np.maximum.reduceat(lcp_pad, idx)[0::2] if len(starts) else np.zeros(0, dtype=np.int64)
    del lcp_pad, idx
    undecided = deepest >= depth
    left = (lens > RUN_MAX) | undecided
    kept = int(lens[left].sum())
    # runs of equal 32-bit keys inside the leftover stretches (k_tie_heads: the first slot of a stretch, or a slot whose 32-bit
    # key differs from the slot before)
    groups = 0
    if kept:
        edge = np.zeros(m + 1, dtype=np.int8)
        edge[starts[left]] = 1
        edge[ends[left]] = -1
        slots = np.flatnonzero(np.cumsum(edge[:m], dtype=np.int8))
        k32 = key[slots] >> np.uint64((nsym - spk) * bits)
        head = np.ones(len(slots), dtype=bool)
        head[1:] = (slots[1:] != slots[:-1] + 1) | (k32[1:] != k32[:-1])
        groups = int(head.sum())
    return {
        "m": m, "bits": bits, "symbols_per_key": spk, "key_symbols": nsym, "depth": depth,
        "tied": int(tied.sum()), "starts": starts, "lens": lens, "undecided": undecided, "left": left,
        "kept": kept, "groups": groups, "small_groups_pay": kept > 0 and groups * 4 >= kept,
    }


def crossing(w, block):
    """Stretches longer than RUN_MAX that cross a multiple of `block` slots."""
    s, e = w["starts"], w["starts"] + w["lens"] - 1
    return int(((w["lens"] > RUN_MAX) & (s // block != e // block)).sum())


def length_classes(w):
    """Stretches per length class 2-3, 4-8, 9-32, 33-63, >= 64."""
    lens = w["lens"]
    return {c: int(((lens >= lo) & (lens <= hi)).sum())
            for c, lo, hi in (("2-3", 2, 3), ("4-8", 4, 8), ("9-32", 9, 32), ("33-63", 33, 63), (">=64", 64, 1 << 62))}
