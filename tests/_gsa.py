"""Shared pieces of the generalized-suffix-array tests (test_gsa_emu.py on the emulator, test_gpu_gsa.py on the GPU):
random document collections, the naive query scan, and the comparison of an engine's table with the definition."""
import ctypes
import os
import random
import subprocess

import numpy as np

from suffix_amd import GeneralizedSuffixTable, SuffixTable

HERE = os.path.dirname(os.path.abspath(__file__))
ALPHABETS = [b"a", b"ab", b"\x00\xff", b"ab\x00\xff"]


def random_collection(rng, max_docs=64, max_len=24):
    """1..max_docs documents over a 1-, 2- or 4-byte alphabet (NUL and 0xFF among them), with empty documents,
    prefixes of earlier documents and exact duplicates placed anywhere (so plain rank != document order)."""
    m = rng.randint(1, max_docs)
    alpha = rng.choice(ALPHABETS)
    docs = []
    for _ in range(m):
        x = rng.random()
        if docs and x < 0.2:
            docs.append(rng.choice(docs))                                   # exact duplicate
        elif docs and x < 0.35:
            d = rng.choice(docs)
            docs.append(d[:rng.randint(0, len(d))])                          # prefix of another document
        elif x < 0.42:
            docs.append(b"")
        else:
            docs.append(bytes(rng.choice(alpha) for _ in range(rng.randint(1, max_len))))
    rng.shuffle(docs)
    return docs


def doc_starts(docs):
    s = np.zeros(len(docs), dtype=np.int64)
    if len(docs) > 1:
        s[1:] = np.cumsum([len(d) for d in docs[:-1]])
    return s


def check_against_naive(eng, docs):
    got = GeneralizedSuffixTable(docs, engine=eng)
    exp = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    for name in ("table", "doc_array", "lcp_lens"):
        assert np.array_equal(getattr(got, name)(), getattr(exp, name)()), (name, docs)
    return got


def naive_matches(docs, q):
    """[(doc, offset)] of q inside single documents (sorted); the empty query has none."""
    if not q:
        return []
    out = []
    for d, doc in enumerate(docs):
        i = doc.find(q)
        while i >= 0:
            out.append((d, i))
            i = doc.find(q, i + 1)
    return out


def boundary_queries(docs, rng, k=6):
    """Strings around the document boundaries of the concatenation: many occur only ACROSS a boundary."""
    text = b"".join(docs)
    starts = doc_starts(docs)
    out = []
    for _ in range(k):
        s = int(starts[rng.randrange(len(starts))])
        a, b = max(0, s - rng.randint(1, 4)), min(len(text), s + rng.randint(1, 4))
        if b > a:
            out.append(text[a:b])
    return out


def check_queries(eng, g, docs, queries):
    res = g.query_batch(queries)
    for k, q in enumerate(queries):
        exp = naive_matches(docs, q)
        s, e = int(res["start"][k]), int(res["end"][k])
        got = sorted(g._pairs(s, e))
        assert got == exp, (q, docs)
        if not exp:
            assert (s, e) == (0, 0) and not res["found"][k] and int(res["any"][k]) == 0xFFFFFFFF, q
        else:
            assert res["found"][k] and int(res["any"][k]) in set(g.table()[s:e].tolist())
        assert int(res["ndocs"][k]) == len({d for d, _ in exp}), (q, docs)
        assert g.documents(q) == sorted({d for d, _ in exp})


def single_doc_matches_plain(eng, text):
    g = GeneralizedSuffixTable([text], engine=eng)
    st = SuffixTable(text, engine=eng)
    assert np.array_equal(g.table(), st.table())
    assert np.array_equal(g.lcp_lens(), st.lcp_lens())
    assert not g.doc_array().any()


def profile_names(eng, fn):
    eng.profile(True)
    eng.profile_reset()
    try:
        fn()
    finally:
        names = {r["name"] for r in eng.profile_report()}
        eng.profile(False)
    return names


def build_checker(out_dir):
    """tests/gsa_check.c -> an executable (the engine-independent checker of large tables)."""
    exe = os.path.join(str(out_dir), "gsa_check")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-o", exe, os.path.join(HERE, "gsa_check.c")])
    return exe


def run_checker(exe, out_dir, text, starts, sa, da, lcp):
    """Writes the five arrays as raw files and runs the checker on them; returns its output line."""
    paths = []
    for name, arr in (("text", np.frombuffer(text, dtype=np.uint8) if isinstance(text, bytes) else text),
                      ("starts", np.asarray(starts, dtype=np.uint64)), ("sa", sa), ("da", da), ("lcp", lcp)):
        p = os.path.join(str(out_dir), name + ".bin")
        np.ascontiguousarray(arr).tofile(p)
        paths.append(p)
    r = subprocess.run([exe, *paths], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data if a.size else 0)
