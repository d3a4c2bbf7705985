"""sg_index_load_reference_ex with device = -1 and the host reader it shares its steps with (ref_index_reader.cpp): the split
into open / decode / assemble changes nothing, the malformed lists tests/test_gpu_index_load.py hands the device decoder are
refused by the host reader, the foreign-but-valid ones are accepted.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

import refindex
from conftest import CARS_DESC, WORDS_DESC, ROOT
from index_load_shapes import (FOREIGN_DESC, FOREIGN_SEGMENTS, MALFORMED_TERM, SG_E_INVALID, assert_same_index, foreign_files, foreign_lists,
                               load_ex, malformed_files, malformed_lists, no_terms_files, pair_twice_files)
from index_store_shapes import SHAPES_DESC, dropped_repeats_files, shapes_files


def _desc(d):
    from suggest_amd import IndexDescription
    return IndexDescription(**d)


def _files(which, tmp_path, golden_dir):
    if which in ("cars", "words_subset"):
        return _desc(CARS_DESC if which == "cars" else WORDS_DESC), os.path.join(golden_dir, "db", which + ".hd"), os.path.join(golden_dir, "db", which + ".dl")
    if which == "shapes":
        _, _, hd, dl = shapes_files(tmp_path, golden_dir)
        return _desc(SHAPES_DESC), hd, dl
    if which == "dropped_repeats":
        d, hd, dl = dropped_repeats_files(tmp_path, golden_dir)
        return _desc(d), hd, dl
    hd, dl, _ = foreign_files(tmp_path, golden_dir)
    return _desc(FOREIGN_DESC), hd, dl


@pytest.mark.parametrize("which", ["cars", "words_subset", "shapes", "dropped_repeats", "foreign"])
def test_ex_on_the_host_is_the_host_reader(which, tmp_path, golden_dir):
    from suggest_amd import NGramIndex
    desc, hd, dl = _files(which, tmp_path, golden_dir)
    assert_same_index(load_ex(hd, dl, desc, -1), NGramIndex.from_reference_files(hd, dl, desc, upload=False))


# sg_index_digest of the fixtures as the reader gave them before it was split into steps (taken with the commit before)
PARENT_DIGESTS = {
    "cars": (0x7166cc43fb19a9bc, 0xed624719801d7948, 0x97b2dd61b6888f6a, 0x0e5c2f6c83152db7),
    "words_subset": (0xd6c391a23dac51a6, 0xc48ae01b49fe8480, 0xe134f9dbd263ce51, 0xa60eccbc0660b19e),
    "shapes": (0x251869b416b2c3c5, 0xa3b76d092f2b3db6, 0xba6ad30aec75a66c, 0xfabda63cdad32505),
}


@pytest.mark.parametrize("which", sorted(PARENT_DIGESTS))
def test_digests_of_the_fixtures_are_what_they_were(which, tmp_path, golden_dir):
    from suggest_amd import NGramIndex
    desc, hd, dl = _files(which, tmp_path, golden_dir)
    assert NGramIndex.from_reference_files(hd, dl, desc, upload=False).digest() == PARENT_DIGESTS[which]
    assert load_ex(hd, dl, desc, -1).digest() == PARENT_DIGESTS[which]


@pytest.mark.parametrize("name", sorted(malformed_lists()))
def test_host_reader_refuses_the_malformed_lists(name, tmp_path, golden_dir):
    from suggest_amd import NGramIndex, _lib
    hd, dl = malformed_files(tmp_path, golden_dir, name)
    for load in (lambda: NGramIndex.from_reference_files(hd, dl, _desc(CARS_DESC), upload=False), lambda: load_ex(hd, dl, _desc(CARS_DESC), -1)):
        with pytest.raises(_lib.SuggestHipError) as e:
            load()
        assert e.value.code == SG_E_INVALID
        assert "'%s'" % MALFORMED_TERM.decode() in str(e.value)


def test_malformed_list_in_front_is_all_that_is_wrong(tmp_path, golden_dir):
    """the splice itself: with a well-formed list in front the files load, and the other lists are those of cars"""
    from index_load_shapes import write_raw_index
    from suggest_amd import NGramIndex
    _, indices, terms = refindex.read_header(os.path.join(golden_dir, "db", "cars.hd"))
    cars = open(os.path.join(golden_dir, "db", "cars.dl"), "rb").read()
    good = refindex.encode_vb([4, 9, 12])
    hd, dl = str(tmp_path / "good.hd"), str(tmp_path / "good.dl")
    write_raw_index(hd, dl, indices, [(MALFORMED_TERM, 0, len(good), 0, 3)] + [(t, i, s, p + len(good), n) for t, i, s, p, n in terms], good + cars,
                    os.path.join(golden_dir, "db", "cars.hd"))
    got = NGramIndex.from_reference_files(hd, dl, _desc(CARS_DESC), upload=False).lists()
    assert got.pop((0, MALFORMED_TERM)) == (3, [4, 9, 12])
    assert got == NGramIndex.from_reference_files(os.path.join(golden_dir, "db", "cars.hd"), os.path.join(golden_dir, "db", "cars.dl"), _desc(CARS_DESC), upload=False).lists()


def test_host_reader_accepts_the_foreign_lists(tmp_path, golden_dir):
    from suggest_amd import NGramIndex
    hd, dl, want = foreign_files(tmp_path, golden_dir)
    ix = NGramIndex.from_reference_files(hd, dl, _desc(FOREIGN_DESC), upload=False)
    got = ix.lists()
    assert {k: v[1] for k, v in got.items()} == want                 # size == 0 and indice >= Indices: skipped
    assert ix.stats()["n_segments"] == FOREIGN_SEGMENTS and ix.stats()["n_docs"] == 1 << 32
    for term, indice, raw, data, stored in foreign_lists():
        if stored is None:
            continue
        if term != b"aah":                                            # (there the reader counts the repeat and the dropped one both)
            assert got[(indice, term)][0] == raw, term
        if term in (b"aaa", b"aab", b"aah", b"aaj"):          # what refindex decodes: blocks of 64 at most, no run past 65 535
            back = refindex.decode_list(memoryview(data), raw)
            assert [x for i, x in enumerate(back) if i == 0 or x != back[i - 1]] == stored, term


def test_header_without_terms(tmp_path, golden_dir):
    from suggest_amd import NGramIndex
    hd, dl = no_terms_files(tmp_path, golden_dir)
    for ix in (NGramIndex.from_reference_files(hd, dl, _desc(FOREIGN_DESC), upload=False), load_ex(hd, dl, _desc(FOREIGN_DESC), -1)):
        assert ix.lists() == {} and ix.stats()["n_docs"] == 0 and ix.stats()["n_segments"] == FOREIGN_SEGMENTS


def test_pair_with_two_lists(tmp_path, golden_dir):
    from suggest_amd import NGramIndex
    hd, dl, want = pair_twice_files(tmp_path, golden_dir)
    host = NGramIndex.from_reference_files(hd, dl, _desc(FOREIGN_DESC), upload=False)
    assert host.lists() == want
    assert_same_index(load_ex(hd, dl, _desc(FOREIGN_DESC), -1), host)


def test_load_times_hook(golden_dir):
    from suggest_amd import _lib
    L = _lib.lib()
    load_ex(os.path.join(golden_dir, "db", "cars.hd"), os.path.join(golden_dir, "db", "cars.dl"), _desc(CARS_DESC), -1)
    out = (C.c_double * 8)(*([-1.0] * 8))
    assert L.sg_debug_index_load_times(out, 7) == 0
    read, parse, h2d, decode, d2h, assemble, whole = list(out)[:7]
    assert h2d == 0 and d2h == 0 and min(read, parse, decode, assemble) >= 0 and out[7] == -1.0
    assert 0 < read + parse + decode + assemble <= whole
    assert L.sg_debug_index_load_times(out, 2) == 0 and L.sg_debug_index_load_times(None, 7) == SG_E_INVALID


def test_python_route_argument(golden_dir):
    """from_reference_files(decode_device=-1) goes through sg_index_load_reference_ex; None is the call it always made"""
    from suggest_amd import NGramIndex
    hd, dl = os.path.join(golden_dir, "db", "cars.hd"), os.path.join(golden_dir, "db", "cars.dl")
    assert_same_index(NGramIndex.from_reference_files(hd, dl, _desc(CARS_DESC), upload=False, decode_device=-1),
                      NGramIndex.from_reference_files(hd, dl, _desc(CARS_DESC), upload=False))


def test_go_shim_passes_as_many_arguments_as_the_header_declares():
    """go/suggesthip/suggesthip.go has never met a Go compiler: the new call passes as many arguments as the header declares"""
    header = open(os.path.join(ROOT, "include", "suggest_hip.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "suggesthip", "suggesthip.go"), encoding="utf-8").read()
    decl = re.search(r"\bint sg_index_load_reference_ex\(([^;]*)\);", header).group(1)
    at = go.index("C.sg_index_load_reference_ex(") + len("C.sg_index_load_reference_ex(")
    depth, n = 0, 1
    while depth >= 0:                                                 # to the call's own closing bracket
        ch = go[at]
        at += 1
        depth += ch in "([{"
        depth -= ch in ")]}"
        n += ch == "," and depth == 0
    assert n == decl.count(",") + 1
    assert "func OpenReference(hdPath, dlPath string, d suggest.IndexDescription, device, decodeDevice int) (*Index, error)" in go


def test_host_reader_compiles_without_hip(tmp_path):
    """ref_index_reader.cpp holds the three steps of a load and the host decoders: plain C++"""
    src = os.path.join(ROOT, "suggest_amd", "csrc", "ref_index_reader.cpp")
    subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-c", src, "-o", str(tmp_path / "ref_index_reader.o")], check=True, capture_output=True, text=True)
