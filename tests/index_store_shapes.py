"""Shared by tests/test_index_store_cpu.py and tests/test_gpu_index_store.py: the edge shapes of a saved index, a run-aware
restatement of roaring's portable serialisation (refindex.encode_roaring writes no run containers), and the comparisons of
saved <name>.hd / <name>.dl files with the reference's own bytes.  The yardsticks are the fixtures under golden/db and the
Python encoders, never the library under test."""
import os
import struct
import subprocess

import refindex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES_DESC = dict(ngram_size=3, wrap=("$", "$"), pad="$", alphabet=("english", "$"))
SHAPES_SEGMENTS = 8


def encode_roaring_runs(values):
    """roaring v0.5.5 WriteTo after RunOptimize over ascending distinct values: per high-16 key a run container when
    2 + 4 * runs <= min(8192, 2 * cardinality) (ties go to the run), else an array up to 4096 values, else a bitmap."""
    cont = {}
    for v in values:
        cont.setdefault(v >> 16, []).append(v & 0xFFFF)
    keys = sorted(cont)
    n = len(keys)
    bodies, is_run = [], []
    for k in keys:
        vals = cont[k]
        runs = []
        for v in vals:
            if runs and runs[-1][0] + runs[-1][1] + 1 == v:
                runs[-1][1] += 1
            else:
                runs.append([v, 0])
        c, r = len(vals), len(runs)
        if 2 + 4 * r <= min(8192, 2 * c):
            is_run.append(True)
            bodies.append(struct.pack("<H", r) + b"".join(struct.pack("<HH", s, l) for s, l in runs))
        elif c <= 4096:
            is_run.append(False)
            bodies.append(struct.pack("<%dH" % c, *vals))
        else:
            is_run.append(False)
            words = [0] * 1024
            for v in vals:
                words[v >> 6] |= 1 << (v & 63)
            bodies.append(struct.pack("<1024Q", *words))
    if any(is_run):
        flags = bytearray((n + 7) // 8)
        for i, f in enumerate(is_run):
            if f:
                flags[i // 8] |= 1 << (i % 8)
        head = struct.pack("<I", 12347 | (n - 1) << 16) + bytes(flags)
        offsets = n >= 4
    else:
        head = struct.pack("<II", 12346, n)
        offsets = True
    head += b"".join(struct.pack("<HH", k, len(cont[k]) - 1) for k in keys)
    if offsets:
        off = len(head) + 4 * n
        for b in bodies:
            head += struct.pack("<I", off)
            off += len(b)
    return head + b"".join(bodies)


def encode_list(raw_len, stored):
    """the bytes Writer.Commit gives a list: `stored` holds the repeats for VB / skip lists, distinct docIDs for roaring"""
    if raw_len <= 65:
        return refindex.encode_vb(stored)
    if raw_len <= 256:
        return refindex.encode_skipping(stored)
    return encode_roaring_runs(sorted(set(stored)))


def _repeats(n_raw, at, step=4, first=3, times=1):
    """n_raw ascending docIDs in which the value at every position of `at` repeats its predecessor"""
    raw, d = [], first
    while len(raw) < n_raw:
        if raw and len(raw) in at:
            raw.extend([raw[-1]] * min(times, n_raw - len(raw)))
        else:
            d += step
            raw.append(d)
    return raw


def edge_shapes():
    """-> [(name, raw_len, list as refindex.write_index takes it)]"""
    out = []
    for n in (1, 63, 64, 65, 66, 127, 128, 129, 192, 255, 256, 257):
        out.append(("len%d" % n, n, [7 + 3 * i for i in range(n)]))
    wide, d = [], 0
    for delta in (5, 200, 20000, 3000000, (1 << 28) + 5, 1, 127, 128, 16383, 16384, 2097151, 2097152, (1 << 28) - 1, 1 << 28):
        d += delta
        wide.append(d)
    out.append(("vb_varint_1_to_5_bytes", len(wide), wide))
    skipw = [3 * i + 1 for i in range(60)]
    d = skipw[-1]
    for i in range(40):                                            # wide deltas before, at and after the block boundary (position 64)
        d += (1, 130, 17000, 2100000, (1 << 28) + 9)[i % 5]
        skipw.append(d)
    out.append(("skip_varint_1_to_5_bytes", len(skipw), skipw))
    out.append(("skip_first_delta_5_bytes", 70, [(1 << 31) + 11 * i for i in range(70)]))
    out.append(("vb_repeat_start_end", 43, _repeats(43, (1, 41, 42))))
    out.append(("vb_repeat_63_64", 65, _repeats(65, (64,))))
    out.append(("vb_repeat_start_63_64", 65, _repeats(65, (1, 2, 64))))
    out.append(("skip_repeat_start_boundary_end", 150, _repeats(150, (1, 64, 128, 149))))
    out.append(("skip_repeat_run_over_boundary", 140, _repeats(140, (62,), times=5)))
    out.append(("skip_only_by_repeats", 66, _repeats(66, (5, 20, 21, 40, 50, 65))))        # 60 stored documents
    assert len(set(out[-1][2])) == 60
    out.append(("skip_256_by_repeats", 256, _repeats(256, (10, 100, 200), times=20)))
    # roaring
    out.append(("roar_two_runs_no_offsets", 70000, list(range(70000))))
    keys0125 = (list(range(100, 400)) + [(1 << 16) + 7 * i for i in range(300)] + list(range(2 << 16, (2 << 16) + 50)) +
                [(5 << 16) + 11 * i + 3 for i in range(40)] + list(range((5 << 16) + 60000, (5 << 16) + 60100)))
    out.append(("roar_runs_keys_0_1_2_5", len(keys0125), keys0125))
    out.append(("roar_bitmap_alternating", 10000, [(3 << 16) + 2 * i for i in range(10000)]))
    sparse5 = [(k << 16) + 97 * i + k for k in (0, 2, 3, 7, 9) for i in range(60)]
    out.append(("roar_sparse_arrays_5_keys", len(sparse5), sparse5))
    edge4096 = [(3 << 16) + 3 * i for i in range(4096)] + [(4 << 16) + 2 * i + 1 for i in range(4097)]
    out.append(("roar_4096_and_4097", len(edge4096), edge4096))
    tie = [5, 6, 7] + [(1 << 16) + 5 * i for i in range(300)]
    out.append(("roar_tie_5_6_7", len(tie), tie))
    ends = [0] + [(1 << 16) + 13 * i for i in range(280)] + [(1 << 16) + 65535] + [(6 << 16) + 65535]
    out.append(("roar_value_0_and_65535", len(ends), ends))
    out.append(("roar_full_container_and_bitmap_tail", 65536 + 5000, list(range(1 << 16, 2 << 16)) + [(2 << 16) + 3 * i for i in range(5000)]))
    dropped = [9 * i + 2 for i in range(200)]
    out.append(("roar_dropped_repeats_short", 300, dropped))       # raw > 256 > stored: PostingListLen survives
    many = [(k << 16) + 3 for k in range(0, 300)]
    out.append(("roar_300_containers_of_one", len(many), many))
    return out


def shape_lists():
    """{(indice, term): (raw_len, list)} for refindex.write_index and the names of the shapes by key"""
    letters = "abcdefghijklmnopqrstuvwxyz"
    lists, names = {}, {}
    for i, (name, raw_len, post) in enumerate(edge_shapes()):
        key = (i % SHAPES_SEGMENTS, ("q" + letters[i // 26] + letters[i % 26]).encode())
        lists[key] = (raw_len, post)
        names[key] = name
    return lists, names


def type_prefix(hd_bytes):
    """the bytes of a gob header in front of its value message: the type definitions"""
    g = refindex._Gob(memoryview(hd_bytes))
    while g.i < len(hd_bytes):
        start = g.i
        n = g.uint()
        end = g.i + n
        if g.int_() >= 0:
            return bytes(hd_bytes[:start])
        g.i = end
    raise ValueError("no value message")


def check_saved(hd, dl, expected, names=None):
    """The saved files against expected = {(indice, term): (raw_len, bytes)}: every list's size, raw length and bytes, and the
    positions, in header order, tile [0, len(dl)) without a gap or an overlap.  `expected` may name fewer lists than were saved."""
    version, indices, terms = refindex.read_header(hd)
    assert version == "v5.1"
    data = open(dl, "rb").read()
    at, seen = 0, set()
    for term, indice, size, pos, length in terms:
        assert pos == at and size > 0, (term, indice, pos, at)
        at += size
        want = expected.get((indice, term))
        if want is None:
            continue
        seen.add((indice, term))
        what = (names or {}).get((indice, term), (indice, term))
        assert length == want[0], what
        assert size == len(want[1]), (what, size, len(want[1]))
        assert data[pos:pos + size] == want[1], what
    assert at == len(data)
    assert seen == set(expected), sorted(set(expected) - seen)[:5]
    return indices, terms


def fixture_lists(golden_dir, name):
    """{(indice, term): (raw_len, bytes)} of a fixture under golden/db"""
    hd, dl = os.path.join(golden_dir, "db", name + ".hd"), os.path.join(golden_dir, "db", name + ".dl")
    _, _, terms = refindex.read_header(hd)
    data = open(dl, "rb").read()
    return {(indice, term): (length, data[pos:pos + size]) for term, indice, size, pos, length in terms}


def dropped_repeats_files(tmp_path, golden_dir):
    """the index of test_gpu_multi.py::test_reference_built_index_with_dropped_repeats: a roaring list with raw > 256 and raw > stored"""
    desc = dict(ngram_size=3, wrap=("$", "$"), pad="$", alphabet=("english", "$"))
    letters = "abcdefghijklmnopqrstuvwxyz"
    docs = [("ab-ab.%s%s" % (letters[i // 26], letters[i % 26])).encode() for i in range(300)]
    docs += [("xy %s%s zz" % (letters[i % 26], letters[i // 26])).encode() for i in range(120)] + [b"ab-ab", b"abab", b"ab ab ab"]
    import oracle
    ora = oracle.OracleIndex(docs, **desc)
    lists = ora.lists()
    assert any(raw > 256 and raw > len(post) for raw, post in lists.values())
    hd, dl = str(tmp_path / "t.hd"), str(tmp_path / "t.dl")
    refindex.write_index(hd, dl, ora.n_segments, lists, os.path.join(golden_dir, "db", "words_subset.hd"))
    return desc, hd, dl


def shapes_files(tmp_path, golden_dir):
    lists, names = shape_lists()
    hd, dl = str(tmp_path / "shapes.hd"), str(tmp_path / "shapes.dl")
    refindex.write_index(hd, dl, SHAPES_SEGMENTS, lists, os.path.join(golden_dir, "db", "words_subset.hd"))
    return lists, names, hd, dl


def check_shapes(tmp_path, golden_dir, device):
    """every edge shape, laid down with refindex.write_index, loaded, saved on `device`: the Python encoders' bytes, and
    refindex.read_index gives the lists back"""
    from suggest_amd import IndexDescription, NGramIndex
    lists, names, hd, dl = shapes_files(tmp_path, golden_dir)
    ix = NGramIndex.from_reference_files(hd, dl, IndexDescription(**SHAPES_DESC), upload=False)
    hd2, dl2 = str(tmp_path / "shapes_saved.hd"), str(tmp_path / "shapes_saved.dl")
    ix.save(hd2, dl2, device=device)
    want = {k: (raw, encode_list(raw, post)) for k, (raw, post) in lists.items()}
    indices, _ = check_saved(hd2, dl2, want, names)
    assert indices == SHAPES_SEGMENTS
    n, back = refindex.read_index(hd2, dl2)
    assert n == SHAPES_SEGMENTS and set(back) == set(lists)
    for k in lists:
        assert back[k] == lists[k], names[k]


CPP = os.path.join(ROOT, "tests", "cpp")


def cpp_program():
    """tests/cpp/index_store_test.cpp, compiled here (tests/cpp/Makefile builds the older programs)"""
    exe = os.path.join(CPP, "_build", "index_store_test")
    src = os.path.join(CPP, "index_store_test.cpp")
    deps = [src, os.path.join(ROOT, "include", "suggest_hip.hpp"), os.path.join(ROOT, "include", "suggest_hip.h"),
            os.path.join(ROOT, "suggest_amd", "libsuggest_hip.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        rocm = os.environ.get("ROCM", "/opt/rocm")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", src, "-o", exe, "-L" + os.path.join(ROOT, "suggest_amd"), "-lsuggest_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "suggest_amd"), "-Wl,-rpath," + rocm + "/lib", "-Wl,-rpath-link," + rocm + "/lib"],
                       check=True, capture_output=True, text=True)
    return exe
