"""Shared by tests/test_lm_mph_cpu.py, tests/test_lm_ngrams_cpu.py and tests/test_gpu_lm_store.py: generated vocabularies and
corpora, the hand-written models, and the comparisons of saved <k>-gm files.  The yardsticks are the reference's own fixture
files under golden/lm, the files the host count builder (LanguageModel.build_files) writes from the same text, tests/mph_ref.py
and, for the device writer, the host writer's files — never the code under test."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM_DIR = os.path.join(ROOT, "tests", "golden", "lm")
CPP = os.path.join(ROOT, "tests", "cpp")
ALPHA_WIDE = ("english", "russian", "numbers", "-'")
ORDERS = (1, 3, 8)
COUNT_EDGES = (1, 9, 10, 99, 100, 999999, 1000000, 4294967295)
SG_E_INVALID, SG_E_UNSUPPORTED = -1, -2


def model_part(data):
    """the prefix of a .lm file that holds the model: version, order, the levels"""
    assert data[:5] == b"0.0.2"
    order, pos = data[5], 6
    for _ in range(order):
        nl = data.index(b"\n", pos)
        cs, vs, _total = (int(x) for x in data[pos:nl].split())
        pos = nl + 1 + cs + vs
    return data[:pos]


def same_model(a, b, what=""):
    assert int(a.order) == int(b.order), what
    assert list(a.words()) == list(b.words()), what
    for i in range(int(a.order)):
        (ac, av, at), (bc, bv, bt) = a.level(i), b.level(i)
        assert np.array_equal(ac, bc), (what, "containers", i)
        assert np.array_equal(av, bv), (what, "values", i)
        assert at == bt, (what, "total", i)


def gen_vocab(n, seed=5):
    """n distinct words (bytes): ASCII and Cyrillic, one of a single byte and (from two words on) one of 300 bytes"""
    rnd = np.random.RandomState(seed)
    latin, cyr = "abcdefghijklmnopqrstuvwxyz", "абвгдежзиклмнопрстуфхцчшщэюя"
    out, seen = [], set()
    if n >= 1:
        out.append(b"q")
    if n >= 2:
        out.append(("z" * 100 + "я" * 100).encode())
        assert len(out[-1]) == 300
    seen.update(out)
    while len(out) < n:
        letters = cyr if rnd.randint(0, 3) == 0 else latin
        w = "".join(letters[int(i)] for i in rnd.randint(0, len(letters), size=int(rnd.randint(2, 9)))).encode()
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def write_vocab_model(directory, words):
    """an order-1 model whose word ids are the positions in `words` (id_order="lines")"""
    with open(os.path.join(directory, "1-gm"), "wb") as f:
        f.write(b"".join(w + b"\t%d\n" % (i % 7 + 1) for i, w in enumerate(words)))


def corpus_20k(seed=3):
    """about 20 000 tokens: Zipf-distributed words, English and Cyrillic, mixed case, sentences of 1 .. 14 words"""
    rnd = np.random.RandomState(seed)
    stems = ["ba", "ca", "mi", "lo", "Tre", "ква", "ЗИ", "сто", "x-", "don'"]
    ends = ["n", "t", "nd", "rk", "й", "ла", "7", "s", "ять", "o"]
    vocab = [s + e for s in stems for e in ends]
    lines, n = [], 0
    while n < 20000:
        k = int(rnd.randint(1, 15))
        lines.append(" ".join(vocab[int(i)] for i in rnd.zipf(1.3, size=k) % len(vocab)))
        n += k
    return ("\n".join(lines) + "\n").encode()


def tile_corpus(m):
    """one sentence of m distinct words: at order 3 the levels hold m + 2, m + 1 and m entries"""
    return (" ".join("w%03d" % i for i in range(m)) + "\n").encode()


def long_word_corpus():
    """six words of 300 bytes in sentences of 9 .. 12 words: at order 8 a line is about 2.4 KB"""
    rnd = np.random.RandomState(8)
    vocab = [(chr(ord("a") + i) * 299 + "x") for i in range(6)]
    return ("\n".join(" ".join(vocab[int(i)] for i in rnd.randint(0, 6, size=int(rnd.randint(9, 13)))) for _ in range(12)) + "\n").encode()


def write_counts_model(directory):
    """order 2, written by hand: every count at which the number of decimal digits changes, and the largest"""
    words = ["w%d" % i for i in range(len(COUNT_EDGES))]
    with open(os.path.join(directory, "1-gm"), "w") as f:
        f.write("".join("%s\t%d\n" % (w, c) for w, c in zip(words, reversed(COUNT_EDGES))))
    with open(os.path.join(directory, "2-gm"), "w") as f:
        f.write("".join("%s %s\t%d\n" % (words[i], words[(i * 3 + 1) % len(words)], c) for i, c in enumerate(COUNT_EDGES)))


def gm_lines(directory, k):
    data = open(os.path.join(directory, "%d-gm" % k), "rb").read()
    assert data == b"" or data.endswith(b"\n")
    return data.split(b"\n")[:-1]


def gm_files(directory, order):
    return [open(os.path.join(directory, "%d-gm" % k), "rb").read() for k in range(1, order + 1)]


def check_ngram_files(model, directory, want_dir, alphabet, start="<S>", end="</S>"):
    """the <k>-gm of `directory` hold the lines of `want_dir` (any order), and load back as `model` array for array"""
    from suggest_amd.spell import LanguageModel
    order = int(model.order)
    for k in range(1, order + 1):
        got = gm_lines(directory, k)
        assert sorted(got) == sorted(gm_lines(want_dir, k)), k
        assert len(got) == len(model.level(k - 1)[1]), k
    assert not os.path.exists(os.path.join(directory, "%d-gm" % (order + 1)))
    same_model(LanguageModel(str(directory), order, start, end, alphabet, id_order="lines"), model, "reload")


def store_times():
    import ctypes as C
    from suggest_amd import _lib
    out = (C.c_double * 4)()
    _lib.check(_lib.lib().sg_debug_lm_store_times(out))
    return [float(x) for x in out]


def cpp_program():
    """tests/cpp/lm_store_test.cpp with the host sources it tests, compiled here under AddressSanitizer and
    UndefinedBehaviorSanitizer (tests/cpp/Makefile builds the older programs): a stand-alone program, no library loaded"""
    exe = os.path.join(CPP, "_build", "lm_store_test")
    csrc = os.path.join(ROOT, "suggest_amd", "csrc")
    srcs = [os.path.join(CPP, "lm_store_test.cpp")] + [os.path.join(csrc, f) for f in ("lm_store.cpp", "lm.cpp", "host_index.cpp")]
    deps = srcs + [os.path.join(csrc, "sg_internal.h"), os.path.join(ROOT, "include", "suggest_hip.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        flags = ["-std=c++17", "-O0", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
        objs = [exe + "_%d.o" % i for i in range(len(srcs))]
        jobs = [subprocess.Popen(["g++"] + flags + ["-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                for src, obj in zip(srcs, objs)]                                     # the four sources side by side
        logs = [j.communicate()[0] for j in jobs]
        assert all(j.returncode == 0 for j in jobs), "\n".join(logs)
        subprocess.run(["g++"] + flags + objs + ["-o", exe], check=True, capture_output=True, text=True)
    return exe
