"""The host-only vocabulary core of beast_bpe_train (csrc/bpe_vocab.h), without a GPU: a small
stand-alone program (tests/host/bpe_vocab_check.cpp, built here with the host compiler) builds
the alphabet, the token hashes and replays a merge log; the Python trainer's build_alphabet,
token_hashes and replay_log, and HF's recorded vocabularies (tests/golden/bpe_hf.json), say what
it must print."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_json, load_npz

CASES = ["skew/2048", "repeat700/2048", "runs/700", "rand256/700", "wide3000/300"]
FAULT_OUT_OF_RANGE, FAULT_DISAGREES = 1, 2


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(present, specials, log) -> the program's parsed output."""
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "the host C++ compiler (g++) is needed, as for the oracle"
    d = tmp_path_factory.mktemp("bpe_vocab")
    exe = str(d / "bpe_vocab_check")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-O1", "-I", os.path.join(REPO, "beast_tokenizer_amd", "csrc"),
                        os.path.join(REPO, "tests", "host", "bpe_vocab_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-4000:]   # -Wall clean

    def unhex(h):
        return "" if h == "-" else bytes.fromhex(h).decode("utf-8")

    def run(present, specials, log):
        path = str(d / "case.txt")
        with open(path, "w") as f:
            f.write(f"{len(present)}\n{''.join('1' if p else '0' for p in present)}\n{len(specials)}\n")
            f.writelines(t.encode("utf-8").hex() + "\n" for t in specials)
            f.write(f"{len(log)}\n")
            f.writelines(" ".join(str(int(v)) for v in e) + "\n" for e in log)
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        lines = iter(r.stdout.split("\n"))
        out = {}
        n = int(next(lines).split()[1])
        rows = [next(lines).split() for _ in range(n)]
        out["id2str"] = [unhex(r[0]) for r in rows]
        out["h"], out["pw"], out["tlen"] = ([int(r[k]) for r in rows] for k in (1, 2, 3))
        out["max_tlen"] = int(next(lines).split()[1])
        out["byte2id"] = [int(v) for v in next(lines).split()[1:]]
        out["capacity"] = int(next(lines).split()[1])
        out["bad"], out["fault"] = (int(v) for v in next(lines).split()[1:])
        out["vocab"] = [unhex(next(lines)) for _ in range(int(next(lines).split()[1]))]
        out["merges"] = [tuple(int(v) for v in next(lines).split()) for _ in range(int(next(lines).split()[1]))]
        return out
    return run


def _presence(rows):
    mn = int(rows.min())
    present = np.zeros(int(rows.max()) - mn + 1, dtype=bool)
    present[np.unique(rows) - mn] = True
    return present


def _python_replay(id2str, str2id, log):
    """bpe_train.replay_log on its Python loop (not the C++ fast path)."""
    import beast_tokenizer_amd.beast_bspline_tokenizer as bt
    from beast_tokenizer_amd import bpe_train
    saved, bt._FAST = bt._FAST, False
    try:
        return bpe_train.replay_log(id2str, str2id, log)
    finally:
        bt._FAST = saved


def _check_alphabet(out, present, specials):
    from beast_tokenizer_amd import bpe_train
    id2str, str2id, byte2id = bpe_train.build_alphabet(present, [chr(i) for i in range(len(present))], specials)
    assert out["id2str"] == id2str
    assert out["byte2id"] == byte2id.tolist()
    h, pw = bpe_train.token_hashes(id2str)
    assert out["h"] == h.tolist() and out["pw"] == pw.tolist()
    assert out["tlen"] == [len(t) for t in id2str]
    assert out["max_tlen"] == max(len(t) for t in id2str)
    return id2str, str2id


@pytest.mark.parametrize("case", CASES)
def test_alphabet_hashes_and_replay_match_python_and_hf(case, check):
    """Per golden case, presence taken from the corpus: the alphabet (id2str, byte2id) is
    build_alphabet's, tlen and the hashes are len(s) and token_hashes', and HF's merges replayed as
    an (a, b, nid, reused) log give HF's vocabulary and merges exactly."""
    from beast_tokenizer_amd import bpe_train
    cname, vs = case.split("/")
    ref = load_json("bpe_hf.json")[case]
    present = _presence(load_npz("bpe_corpora.npz")[cname].astype(np.int64))
    base, _, _ = bpe_train.build_alphabet(present, [chr(i) for i in range(len(present))], ())
    known, log = set(base), []
    for sa, sb in ref["merges"]:
        log.append((ref["vocab"][sa], ref["vocab"][sb], ref["vocab"][sa + sb], int(sa + sb in known)))
        known.add(sa + sb)
    out = check(present, (), log)
    id2str, str2id = _check_alphabet(out, present, ())
    assert out["capacity"] == bpe_train.loop_log_capacity(len(base) + len(log), len(base))
    assert (out["bad"], out["fault"]) == (-1, 0)
    assert {t: i for i, t in enumerate(out["vocab"])} == ref["vocab"] and len(out["vocab"]) == len(ref["vocab"])
    assert [[out["vocab"][a], out["vocab"][b]] for a, b in out["merges"]] == ref["merges"]
    if cname == "wide3000":   # three-byte UTF-8, 3000 base tokens, no merge
        assert len(present) == 3000 and not log and any(len(t.encode()) == 3 for t in out["id2str"])
    merges = _python_replay(id2str, str2id, log)
    assert id2str == out["vocab"] and [list(m) for m in merges] == ref["merges"]


def test_alphabet_with_special_tokens(check):
    """Special tokens come first, a repeated one once."""
    present = _presence(load_npz("bpe_corpora.npz")["skew"].astype(np.int64))
    specials = ("<pad>", "<eos>", "<pad>")
    out = check(present, specials, [])
    _check_alphabet(out, present, specials)
    assert out["id2str"][:3] == ["<pad>", "<eos>", "\x00"] and out["vocab"] == out["id2str"]


def test_replay_reports_the_first_bad_entry(check):
    """A good log with id re-use replays as replay_log does; a wrong nid, a wrong reused flag and an
    id past the vocabulary each come back as the index of the bad entry (replay_log: None), the
    vocabulary and merges as the entries before it left them."""
    present = np.zeros(256, dtype=bool)
    present[[0, 233, *range(97, 103)]] = True     # chr(0 .. 255), then byte 0's 'Ā'
    base = check(present, (), [])["id2str"]
    n0 = len(base)
    a, b, c, d = (base.index(ch) for ch in "abcd")
    assert n0 == 257 and base[256] == "Ā" and base[255] == "ÿ"

    def fresh():
        return list(base), {t: i for i, t in enumerate(base)}
    # new tokens ab, abc, Āÿ, dd, dddd, then a merge whose string exists: "a" + "b" re-uses "ab"
    good = [(a, b, n0, 0), (n0, c, n0 + 1, 0), (256, 255, n0 + 2, 0), (d, d, n0 + 3, 0),
            (n0 + 3, n0 + 3, n0 + 4, 0), (a, b, n0, 1)]
    out = check(present, (), good)
    ids, s2i = fresh()
    merges = _python_replay(ids, s2i, good)
    assert (out["bad"], out["fault"]) == (-1, 0) and out["vocab"] == ids
    assert out["vocab"][n0:] == ["ab", "abc", "Āÿ", "dd", "dddd"]
    assert [(ids[x], ids[y]) for x, y in out["merges"]] == merges
    for bad_log, at in (([(a, b, n0 + 1, 0)], 0), ([(a, b, n0, 1)], 0), ([(a, b, n0, 0), (a, b, n0 + 1, 0)], 1)):
        out = check(present, (), bad_log)
        assert (out["bad"], out["fault"]) == (at, FAULT_DISAGREES)
        assert out["vocab"] == base + ["ab"] * at and out["merges"] == [(a, b)] * at
        assert _python_replay(*fresh(), bad_log) is None
    for bad_log, at in (([(a, n0, n0, 0)], 0), ([(a, b, n0, 0), (n0 + 1, a, n0 + 1, 0)], 1), ([(-1, a, n0, 0)], 0)):
        out = check(present, (), bad_log)
        assert (out["bad"], out["fault"]) == (at, FAULT_OUT_OF_RANGE)
        assert out["vocab"] == base + ["ab"] * at
