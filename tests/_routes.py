"""The route matrix: which (symbol width, key, sort route, LCP route) cells the engine has, one text per cell, and what a build of
that text must report.  Engine-agnostic like _cases.py: the CPU run passes the emulator build, the GPU run the product library.

The engine packs a text's bytes into dense symbols of 1 .. 8 bits and chooses, from the packing, the length and the byte counts,
a key (32-bit, 64-bit fixed-width, 64-bit compressed), a sort route (one workgroup, device-wide passes, the hybrid route with or
without oversized sub-buckets) and an LCP route.  `predict` restates the rules that depend on (bytes, n) alone in plain Python --
it never calls the engine -- the table CASES declares one cell per text, REQUIRED lists by hand the cells the table must hold and
EXEMPT those that do not exist or lie beyond 2^28 bytes.  `check_case` builds a text through the three device entry points,
compares every array with the oracle and holds build_stats() and the kernels' profile names to the declared cell; for fixed-width
keys it also holds `active_after_initial` to the witness of _ties.py, because the pipeline heals itself: an initial sort that marks
too much as tied still ends in the right array.

Everything is deterministic: _gen.* with fixed seeds."""
from collections import namedtuple

import numpy as np

import _gen
import _ties

TINY_MAX = 16384                # kTinyMax: texts up to here start in the single-workgroup build ...
TINY_MAX_8 = 4096               # kTinyMaxBytes8: ... which hands a text of more than 16 distinct bytes above this on at once
HYBRID_MIN, HYBRID_MAX = 1 << 25, 1 << 28
HT_MIN = 1 << 16                # compressed keys and the count histogram are considered from here
DIRECT_MIN = 1 << 20            # kDirectMinN: below, the separate LCP entry runs Phi / PLCP without sampling
DIRECT_CAP = 1024               # kDirectCap: a pair that agrees on this many bytes is handed to Phi / PLCP
SAMPLES, SAMPLE_CAP = 1 << 16, 4096     # kSamples adjacent pairs, each LCP capped at kSampleCap
MEAN_DIRECT_MAX, MEAN_WIDE_MIN = 64, 16  # sampled mean LCP: direct pass up to 64 bytes, its 32-byte window from 16
MARGIN = 0.05                   # how far spw * per stays from bits_for(n) + 1 when `per` is a sum of floating-point terms

M_HYBRID = (1 << 25) + 4099     # the smallest odd-sized text of the hybrid route (the last word of the tie mask is partial)
M_DIRECT = (1 << 20) + 7


def bits_for(v):
    """sfx_device.hpp: bits needed for the values 0 .. v (at least 1)."""
    return max(1, int(v).bit_length())


def predict(text):
    """The dispatch rules of build_sa_impl / choose_key / tiny_build_sa_dev / hybrid_size_ok that depend on (bytes, n) only.
    -> dict: sigma, bits, spw, key ('k32' | 'k64': fixed-width or compressed is the code construction's call), key_bits,
    symbols_per_key (of a fixed-width key), sort ('tiny' | 'tiny_handed_on' | 'passes' | 'hybrid': a 'tiny' text with long repeats
    is handed on, a 'hybrid' one gives way or not by its sub-bucket histogram), margin."""
    t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, dtype=np.uint8)
    n = int(t.size)
    counts = np.bincount(t, minlength=256).astype(np.int64)
    return predict_from_counts(counts, n)


def predict_from_counts(counts, n):
    sigma = int((counts > 0).sum())
    bits = bits_for(sigma - 1 if sigma > 1 else 1)
    spw = 32 // bits
    l2 = max(1, bits_for(sigma) - 1)                  # floor(log2 sigma)
    thr = bits_for(n) + 1
    per, margin = float(l2), None
    key32 = spw * l2 >= thr                           # (integers: exact on both sides, a flip point itself is no hair)
    if key32 and sigma > 16 and n >= HT_MIN:
        # the counts decide: the order-0 entropy where it is below floor(log2 sigma)
        q = counts[counts > 0].astype(np.float64) / float(n)
        h0 = float(-(q * np.log2(q)).sum()) if n > 256 else -1.0
        if h0 > 0.0:
            if h0 < l2 - MARGIN / spw:
                per = h0
                margin = abs(spw * h0 - thr)
                assert margin >= MARGIN, f"sigma {sigma}, n {n}: {spw} x {h0:.6f} against {thr} is a hair"
                key32 = spw * h0 >= thr
            elif h0 <= l2 + MARGIN / spw:
                # (the summation order could put the entropy on either side of floor(log2 sigma): both must decide alike)
                margin = abs(spw * h0 - thr)
                assert margin >= MARGIN and (spw * h0 >= thr) == key32, f"sigma {sigma}, n {n}: {spw} x {h0:.6f} against {thr} is a hair"
    key_bits = 32 if key32 else 64
    if n <= TINY_MAX:
        sort = "tiny" if (sigma <= 16 or n <= TINY_MAX_8) else "tiny_handed_on"
    elif key32 and HYBRID_MIN <= n <= HYBRID_MAX and bits * spw >= 24:
        sort = "hybrid"
    else:
        sort = "passes"
    return {"n": n, "sigma": sigma, "bits": bits, "spw": spw, "key": "k32" if key32 else "k64", "key_bits": key_bits,
            "symbols_per_key": spw if key32 else 2 * spw, "per": per, "threshold": thr, "margin": margin, "sort": sort}


def top16_histogram(text):
    """Sub-bucket sizes of the hybrid route (k_hist16_text): suffixes by the top 16 bits of their bits * spw-bit key, zero-padded
    past the end.  -> (largest, suffixes in sub-buckets above 4096)."""
    codes, bits, _ = _ties.codes_of(text)
    m = len(codes)
    nsym = -(-16 // bits)
    padded = np.concatenate([codes, np.zeros(nsym, dtype=np.uint8)])
    hist = np.zeros(1 << 16, dtype=np.int64)
    for a in range(0, m, 1 << 24):
        b = min(m, a + (1 << 24))
        k = np.zeros(b - a, dtype=np.int64)
        for j in range(nsym):
            k = (k << bits) | padded[a + j:b + j]
        hist += np.bincount(k >> (nsym * bits - 16), minlength=1 << 16)
    return int(hist.max()), int(hist[hist > _ties.SLOW].sum())


def sampled_mean(lcp):
    """k_lcp_sample over the oracle's LCP array: the pairs at ranks 1 + j * every, each capped at 4096.  -> (sum, samples)."""
    n = len(lcp)
    samples = min(SAMPLES, n - 1)
    every = (n - 1) // samples
    r = 1 + np.arange(samples, dtype=np.int64) * every
    r = r[r < n]
    return int(np.minimum(np.asarray(lcp)[r].astype(np.int64), SAMPLE_CAP).sum()), samples


def lcp_route_of(sigma, lcp):
    """The route of the separate LCP entry (build_lcp_u32_dev) from the oracle's LCP array.  -> (route, window bytes or None)."""
    n = len(lcp)
    if n < DIRECT_MIN:
        return "plcp_small", None
    total, samples = sampled_mean(lcp)
    if total > MEAN_DIRECT_MAX * samples:
        return "sampled_plcp", None
    window = None
    if sigma > 16:
        mean = total / samples
        assert mean <= 12 or mean >= 20, f"sampled mean LCP {mean:.2f}: too near the 16-byte threshold of the window width"
        window = 32 if total >= MEAN_WIDE_MIN * samples else 16
    capped = int(np.asarray(lcp).max()) >= DIRECT_CAP
    return ("direct_then_plcp" if capped else ("direct_packed" if sigma <= 16 else "direct_raw")), window


# ---- generators -------------------------------------------------------------------------------------------------------------------

def uniform(n, sigma, seed):
    return _gen.uniform_bytes(n, sigma, seed, base=0 if sigma > 190 else 40)


def skewed(n, sigma, seed, ratio):
    """n bytes over `sigma` values with geometric weights ratio^k, drawn through a 65536-entry table from 16-bit pieces of the
    splitmix64 stream."""
    w = ratio ** np.arange(sigma, dtype=np.float64)
    cnt = np.maximum(1, np.floor(w / w.sum() * 65536.0)).astype(np.int64)
    cnt[0] += 65536 - int(cnt.sum())
    assert cnt[0] >= 1
    lut = np.repeat(np.arange(sigma, dtype=np.uint8), cnt)
    u16 = _gen.splitmix64_stream(seed, (n + 3) // 4).view(np.uint16)[:n]
    t = lut[u16]
    t[np.arange(sigma) * (n // sigma)] = np.arange(sigma, dtype=np.uint8)      # (every value at least once, whatever the draw)
    return t + np.uint8(0 if sigma > 190 else 40)


def twins(n, sigma, seed, every):
    """X + X' : X uniform, X' = X with one byte changed every `every` bytes -- nearly every suffix shares ~every / 2 bytes with its
    twin, none more than `every`."""
    h = n // 2
    x = uniform(n - h, sigma, seed)
    y = x[:h].copy()
    y[every // 2::every] ^= 1
    return np.concatenate([x, y])


def long_run(n, sigma, seed, length=1500):
    """Uniform text with one block of `length` bytes planted twice: a low sampled mean, and pairs beyond kDirectCap."""
    t = uniform(n, sigma, seed).copy()
    t[n // 5:n // 5 + length] = t[n // 2:n // 2 + length]
    return t


def doubled(n, sigma, seed):
    x = uniform(n // 2, sigma, seed)
    return np.concatenate([x, x])


def oversized(n, sigma, seed, copies=20000, tail=16):
    """Uniform text with `copies` copies of a block one symbol longer than the 16 top key bits, each followed by `tail` random
    symbols: one sub-bucket above what the LDS sort holds (as test_hybrid_initial_sort_56mb plants for DNA)."""
    bits = bits_for(sigma - 1)
    blk = 16 // bits + 1
    t = uniform(n, sigma, seed).copy()
    rng_bytes = uniform(copies * tail, sigma, seed + 1).reshape(copies, tail)
    head = uniform(blk, sigma, seed + 2)
    block = np.concatenate([np.tile(head, (copies, 1)), rng_bytes], axis=1).reshape(-1)
    t[1_000_000:1_000_000 + block.size] = block
    return t


# ---- the table --------------------------------------------------------------------------------------------------------------------

Case = namedtuple("Case", "name make n cell tags fused where")
"""cell = (bits, key, sort route, LCP route of the separate entry); tags: 'flip_lo' / 'flip_hi' (n - 1 and n of a flip of
choose_key), 'w16' / 'w32' (window of the raw direct pass), 'packed' / 'raw' (which direct pass ran before Phi / PLCP);
fused: the one-call entry finished the LCP from the keys and the pending pairs (lcp_pending, no run of the separate routine);
where: 'emu+gpu' (at most 2^19 bytes), 'gpu', or the id of the existing GPU test that builds this text."""

EMU_MAX = 1 << 19
_TIE = "tests/test_gpu_tie_route.py::test_tie_route_sa_lcp[%s]"


def _c(name, make, n, cell, tags=(), fused=True, where=None):
    return Case(name, make, n, cell, frozenset(tags), fused, where or ("emu+gpu" if n <= EMU_MAX else "gpu"))


def _table():
    t = []
    pow2 = {b: 1 << b for b in range(1, 9)}
    # every width on 32-bit keys through the device-wide passes, Phi / PLCP below 2^20
    for b, sg in pow2.items():
        t.append(_c(f"passes_b{b}", lambda sg=sg, b=b: uniform(20011 + 2 * b, sg, 100 + b), 20011 + 2 * b, (b, "k32", "passes", "plcp_small")))
    # the single-workgroup build, and its hand-over of wider symbols above 4096 bytes
    for b in (1, 2, 3, 4):
        t.append(_c(f"tiny_b{b}", lambda b=b: uniform(5003 + b, pow2[b], 200 + b), 5003 + b, (b, "k32", "tiny", "plcp_small"), fused=False))
    for b in (5, 6, 7, 8):
        t.append(_c(f"handed_b{b}", lambda b=b: uniform(7001 + b, pow2[b], 300 + b), 7001 + b, (b, "k32", "tiny_handed_on", "plcp_small")))
    # n - 1 and n of one flip of choose_key per width (1-bit symbols have none below 2^31)
    for b, sg, e in ((2, 3, 15), (3, 5, 19), (4, 12, 23), (5, 20, 23), (6, 40, 24), (7, 97, 23)):
        lcp = "plcp_small" if e < 20 else ("direct_packed" if sg <= 16 else "direct_raw")
        tags = () if e < 20 or sg <= 16 else ("w16",)
        t.append(_c(f"flip_b{b}_lo", lambda sg=sg, e=e, b=b: uniform((1 << e) - 1, sg, 400 + b), (1 << e) - 1, (b, "k32", "passes", lcp), ("flip_lo",) + tags))
        t.append(_c(f"flip_b{b}_hi", lambda sg=sg, e=e, b=b: uniform(1 << e, sg, 410 + b), 1 << e, (b, "k64", "passes", lcp), ("flip_hi",) + tags))
    # (8-bit symbols: the uniform flip is at 2^27 -- skewed counts, whose entropy term puts it at 2^23)
    t.append(_c("flip_b8_lo", lambda: skewed((1 << 23) - 1, 200, 408, 0.9625), (1 << 23) - 1, (8, "k32", "passes", "direct_raw"), ("flip_lo", "w16")))
    t.append(_c("flip_b8_hi", lambda: skewed(1 << 23, 200, 418, 0.9625), 1 << 23, (8, "k64c", "passes", "direct_raw"), ("flip_hi", "w16")))
    # compressed 64-bit keys per width
    t.append(_c("k64c_b2", lambda: skewed(70001, 3, 502, 0.12), 70001, (2, "k64c", "passes", "plcp_small"), fused=False))   # (0.6 bits a symbol: most suffixes stay tied)
    t.append(_c("k64c_b3", lambda: skewed((1 << 19) + 13, 6, 503, 0.5), (1 << 19) + 13, (3, "k64c", "passes", "plcp_small"), where="gpu"))
    t.append(_c("k64c_b4", lambda: skewed((1 << 23) + 5, 12, 504, 0.6), (1 << 23) + 5, (4, "k64c", "passes", "direct_packed")))
    for b, sg, r in ((5, 20, 0.5), (6, 40, 0.6), (7, 100, 0.7), (8, 200, 0.8)):
        t.append(_c(f"k64c_b{b}", lambda sg=sg, r=r, b=b: skewed(70001 + b, sg, 500 + b, r), 70001 + b, (b, "k64c", "passes", "plcp_small")))
    # the direct LCP pass on packed symbols, every width it takes, and on raw bytes in both window widths
    for b in (1, 2, 3, 4):
        t.append(_c(f"direct_b{b}", lambda b=b: uniform(M_DIRECT, pow2[b], 600 + b), M_DIRECT, (b, "k32", "passes", "direct_packed")))
    t.append(_c("direct_raw_w16", lambda: uniform(M_DIRECT, 64, 611), M_DIRECT, (6, "k32", "passes", "direct_raw"), ("w16",)))
    t.append(_c("direct_raw_w32", lambda: twins(M_DIRECT, 64, 612, 100), M_DIRECT, (6, "k32", "passes", "direct_raw"), ("w32",), fused=False))   # (half the suffixes tied to a twin: rank rounds)
    t.append(_c("direct_then_plcp_packed", lambda: long_run(M_DIRECT, 4, 613), M_DIRECT, (2, "k32", "passes", "direct_then_plcp"), ("packed",)))
    t.append(_c("direct_then_plcp_raw", lambda: long_run(M_DIRECT, 64, 614), M_DIRECT, (6, "k32", "passes", "direct_then_plcp"), ("raw", "w16")))
    t.append(_c("sampled_plcp", lambda: doubled(M_DIRECT + 1, 4, 615), M_DIRECT + 1, (2, "k32", "passes", "sampled_plcp"), fused=False))
    # the hybrid route: tie mode on every width (1, 2 and 4 bits are the texts of test_gpu_tie_route.py), sorted keys with an
    # oversized sub-bucket on 3 bits and on more than 4
    gt = _ties.gpu_texts()
    for b, nm in ((1, "binary"), (2, "planted_dna"), (4, "sigma16")):
        t.append(_c(f"hybrid_ties_b{b}", gt[nm][0], gt[nm][1], (b, "k32", "hybrid_ties", None), where=_TIE % nm))     # (LCP route: not declared, that test compares the arrays only)
    for b in (3, 5, 6, 7, 8):
        lcp, tags = ("direct_packed", ()) if b <= 4 else ("direct_raw", ("w16",))
        t.append(_c(f"hybrid_ties_b{b}", lambda b=b: uniform(M_HYBRID, pow2[b], 700 + b), M_HYBRID, (b, "k32", "hybrid_ties", lcp), tags))
    t.append(_c("hybrid_keys_b3", lambda: oversized(M_HYBRID, 8, 713), M_HYBRID, (3, "k32", "hybrid_keys", "direct_packed")))
    t.append(_c("hybrid_keys_b6", lambda: oversized(M_HYBRID, 64, 716), M_HYBRID, (6, "k32", "hybrid_keys", "direct_raw"), ("w16",)))
    return t


CASES = _table()

# What the table must hold, by hand: (bits, key, sort, lcp, tag), None = whichever.
REQUIRED = (
    [(b, "k32", "passes", None, None) for b in range(1, 9)]
    + [(b, "k32", "hybrid_ties", None, None) for b in range(1, 9)]
    + [(3, "k32", "hybrid_keys", None, None), (6, "k32", "hybrid_keys", None, None)]
    + [(b, "k64", "passes", None, None) for b in range(2, 8)]
    + [(b, "k64c", "passes", None, None) for b in range(2, 9)]
    + [(b, None, "passes", None, f) for b in range(2, 9) for f in ("flip_lo", "flip_hi")]
    + [(b, None, "tiny", None, None) for b in (1, 2, 3, 4)]
    + [(b, None, "tiny_handed_on", None, None) for b in (5, 6, 7, 8)]
    + [(b, None, None, "direct_packed", None) for b in (1, 2, 3, 4)]
    + [(None, None, None, "direct_raw", "w16"), (None, None, None, "direct_raw", "w32")]
    + [(None, None, None, "direct_then_plcp", "packed"), (None, None, None, "direct_then_plcp", "raw")]
    + [(None, None, None, "sampled_plcp", None), (None, None, None, "plcp_small", None)]
)

# Cells that do not exist, or that no text of at most 2^28 bytes (for the 64-bit keys: of at most 2^24 + 1 bytes, the cap this
# matrix sets itself) reaches.  (bits, key, sort) -> reason.
EXEMPT = {
    (1, "k64", "passes"): "32 one-bit symbols fill a 32-bit key for every n < 2^31: 64-bit keys need 2^31 bytes",
    (1, "k64c", "passes"): "as above: a one-bit text never takes 64-bit keys below 2^31 bytes",
    (8, "k64", "passes"): "fixed-width 64-bit keys of 8-bit symbols need counts the code does not pay on (entropy above 7.25 bits) and "
                          "4 x entropy < bits_for(n) + 1: n >= 2^27 (uniform over 129 .. 255 values), past the 2^24 + 1 cap; tried: every "
                          "skew that flips 8-bit symbols below 2^27 compresses (flip_b8_hi is k64c)",
    **{(b, k, s): "the hybrid route takes 32-bit keys only (hybrid_sort_e64_text is the E64 sort's)"
       for b in range(1, 9) for k in ("k64", "k64c") for s in ("hybrid_ties", "hybrid_keys")},
}
# Noted, not cells of this matrix: sigma = 4 on 64-bit keys needs 2^31 bytes (test_config4_virtual_ranks has the virtual form); the
# slices of the range-partitioned build stay DNA-only (another width there costs two 35 s oracle runs).


def provides(case):
    """The (bits, key, sort, lcp, tag) tuples a case stands for."""
    return [case.cell + (tag,) for tag in (None, *sorted(case.tags))]


def satisfied(req, cases):
    return [c.name for c in cases if any(all(r is None or r == p for r, p in zip(req, prov)) for prov in provides(c))]


# ---- one case through an engine --------------------------------------------------------------------------------------------------

def _profiled(eng, device, fn):
    import torch
    eng.profile(True)
    eng.profile_reset()
    out = fn()
    if device != "cpu":
        torch.cuda.synchronize()
    rep = {r["name"]: r for r in eng.profile_report()}
    eng.profile(False)
    return out, rep


def sort_route_of(names):
    if "tiny_sa" in names:
        return "tiny_handed_on" if "groups_reduce" in names else "tiny"
    if "bucket_sort_ties" in names or "bucket_sort_ties_keys" in names:
        return "hybrid_ties" if "tie_direct" in names and "oversize_gather" not in names else "?"
    if "bucket_sort_lds" in names:
        return "hybrid_keys" if "oversize_gather" in names and "tie_direct" not in names else "?"
    return "passes"


def lcp_route_from_names(names):
    if "lcp_sample" not in names:
        return "plcp_small" if "plcp" in names else "?"
    direct = "lcp_windows_packed" in names or "lcp_windows" in names
    if not direct:
        return "sampled_plcp" if "plcp" in names else "?"
    if "plcp" in names:
        return "direct_then_plcp"
    return "direct_packed" if "lcp_windows_packed" in names else "direct_raw"


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def check_case(eng, orc, case, device, arrays=None):
    """One case through build_sa, build_lcp and build_sa_lcp of `eng` on `device`.  arrays: (text, sa, lcp) of the oracle where the
    caller has them already.  -> the profile of the build_sa call (name -> record), its build_stats() and the witness (None
    for the single-workgroup build and for compressed keys)."""
    import torch

    from suffix_amd import device as sdev
    if arrays is None:
        text = np.ascontiguousarray(case.make())
        exp = orc.sais(text)
        arrays = (text, exp, orc.lcp_kasai(text, exp))
    text, exp, want = arrays
    assert len(text) == case.n, (case.name, len(text))
    bits, key, sort, lcp_route = case.cell
    p = predict(text)
    assert p["bits"] == bits, (case.name, p)
    d_text = torch.from_numpy(text).to(device)

    sa, rep = _profiled(eng, device, lambda: sdev.build_sa(d_text, engine=eng))
    st = eng.build_stats()
    assert np.array_equal(_u32(sa), exp), case.name
    del sa
    assert sort_route_of(set(rep)) == sort, (case.name, sorted(rep))

    seen = {"witness": None}

    def stats_say(st, how):
        if sort == "tiny":                      # (the single-workgroup build fills no statistics)
            return
        got_key = "k64c" if "ht_keys" in rep else f"k{st['key_bits']}"
        assert got_key == key and st["key_bits"] == p["key_bits"], (case.name, how, got_key, st, p)
        if key == "k64c":
            return
        assert (st["bits_per_symbol"], st["symbols_per_key"]) == (p["bits"], p["symbols_per_key"]) and p["bits"] == bits, (case.name, how, st, p)
        # every slot the initial sort must leave tied, and no other: the hybrid route's tie mode keys on one more symbol where
        # the suffix index leaves room (keys that fill their 32 bits with symbols of at most 4 bits, SrcText36: not 3-bit symbols)
        nsym = p["symbols_per_key"] + (1 if sort == "hybrid_ties" and bits <= 4 and bits * p["spw"] == 32 else 0)
        if seen["witness"] is None:
            seen["witness"] = _ties.witness(text, exp, want, key_symbols=nsym)
        tied = seen["witness"]["tied"]
        assert st["active_after_initial"] == tied, (case.name, how, st["active_after_initial"], tied)
    stats_say(st, "build_sa")

    d_exp = torch.from_numpy(exp.view(np.int32)).to(device)
    lcp, rep_l = _profiled(eng, device, lambda: sdev.build_lcp(d_text, d_exp, engine=eng))
    assert np.array_equal(_u32(lcp), want), case.name
    del lcp, d_exp
    assert lcp_route_from_names(set(rep_l)) == lcp_route, (case.name, sorted(rep_l))
    route, window = lcp_route_of(p["sigma"], want)
    assert route == lcp_route, (case.name, route)
    if lcp_route == "direct_then_plcp":
        assert ("lcp_windows_packed" in rep_l) == ("packed" in case.tags) and ("lcp_windows" in rep_l) == ("raw" in case.tags), (case.name, sorted(rep_l))
    if window:
        assert f"w{window}" in case.tags, (case.name, window)

    (sa2, lcp2), rep_f = _profiled(eng, device, lambda: sdev.build_sa_lcp(d_text, engine=eng))
    assert np.array_equal(_u32(sa2), exp), case.name
    assert np.array_equal(_u32(lcp2), want), case.name
    del sa2, lcp2
    fused = "lcp_pending" in rep_f and "plcp" not in rep_f and "lcp_sample" not in rep_f
    assert fused == case.fused, (case.name, sorted(rep_f))
    assert sort_route_of(set(rep_f)) == sort, (case.name, sorted(rep_f))
    stats_say(eng.build_stats(), "build_sa_lcp")
    return rep, st, seen["witness"]
