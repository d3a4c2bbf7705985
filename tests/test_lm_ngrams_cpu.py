"""LanguageModel.save_ngrams with the host writer (sg_lm_store_google, device = -1): a model written as the Google n-gram files
<dir>/<k>-gm the reference's build-lm step reads (pkg/lm/ngram_writer.go:12,51-60).  Held against the reference's own fixture
files under golden/lm and the files the host count builder writes from the same text, as sorted lines (the reference's line
order is Go-map random), and against the model itself after a reload.  No GPU needed; tests/test_gpu_lm_store.py holds the
device writer against this one."""
import os
import re
import subprocess

import pytest

from lm_store_shapes import (ALPHA_WIDE, COUNT_EDGES, LM_DIR, ORDERS, ROOT, SG_E_INVALID, SG_E_UNSUPPORTED, check_ngram_files, corpus_20k,
                             cpp_program, gm_lines, store_times, write_counts_model)

FIXTURE_ALPHA = ("english", "russian", "numbers", "-.")


@pytest.mark.parametrize("id_order", ("count", "lines"))
def test_fixture_model_gives_the_reference_files_back(id_order, tmp_path):
    from suggest_amd.spell import LanguageModel
    src = LanguageModel(LM_DIR, id_order=id_order)
    src.save_ngrams(str(tmp_path), device=-1)
    check_ngram_files(src, tmp_path, LM_DIR, FIXTURE_ALPHA)
    assert [ln.split(b"\t")[0] for ln in gm_lines(tmp_path, 1)] == src.words()       # 1-gm: a line per word in id order
    t = store_times()
    assert t[0] == 0 and t[2] == 0 and t[1] >= 0 and t[3] > 0


@pytest.fixture(scope="module")
def corpus_files(tmp_path_factory):
    """the count files the host builder writes from the 20 000-token text, per order"""
    from suggest_amd.spell import LanguageModel
    text = corpus_20k()
    assert 20000 <= len(text.split()) < 20020
    out = {}
    for order in ORDERS:
        d = tmp_path_factory.mktemp("built%d" % order)
        LanguageModel.build_files(text, str(d), order, "<S>", "</S>", ALPHA_WIDE, ("\n",))
        out[order] = str(d)
    return out


@pytest.mark.parametrize("order", ORDERS)
def test_generated_corpus(order, corpus_files, tmp_path):
    from suggest_amd.spell import LanguageModel
    src = LanguageModel(corpus_files[order], order, "<S>", "</S>", ALPHA_WIDE, id_order="count")
    assert len(src.level(order - 1)[1]) > 100
    assert any(w[0] >= 0x80 for w in src.words())                               # Cyrillic words are there
    src.save_ngrams(tmp_path, device=-1)
    check_ngram_files(src, tmp_path, corpus_files[order], ALPHA_WIDE)


def test_digit_boundaries(tmp_path):
    from suggest_amd.spell import LanguageModel
    src_dir, out = tmp_path / "src", tmp_path / "out"
    src_dir.mkdir(); out.mkdir()
    write_counts_model(str(src_dir))
    src = LanguageModel(str(src_dir), 2, "<S>", "</S>", ("english", "numbers"), id_order="lines")
    src.save_ngrams(out, device=-1)
    check_ngram_files(src, out, src_dir, ("english", "numbers"))
    assert sorted(int(ln.split(b"\t")[1]) for ln in gm_lines(out, 2)) == sorted(COUNT_EDGES)
    assert open(str(out / "1-gm"), "rb").read() == open(str(src_dir / "1-gm"), "rb").read()


def _refused(lm, directory, level):
    from suggest_amd import _lib
    with pytest.raises(_lib.SuggestHipError) as e:
        lm.save_ngrams(directory, device=-1)
    assert e.value.code == SG_E_UNSUPPORTED and ("level %d" % level) in str(e.value)
    assert os.listdir(str(directory)) == []


def test_models_that_cannot_be_spelled_are_refused_and_no_file_is_created(tmp_path):
    from suggest_amd.spell import LanguageModel
    from test_lm_orders_cpu import write_orphan_model
    out = tmp_path / "out"
    out.mkdir()
    orphan = tmp_path / "orphan"
    orphan.mkdir()
    write_orphan_model(str(orphan), 8)                                          # its 1-gm lists "a" twice
    _refused(LanguageModel(str(orphan), 8, "<S>", "</S>", ("english", "numbers"), id_order="lines"), out, 1)
    nocontext = tmp_path / "nocontext"                                           # a 3-gram whose 2-gram prefix is in no file
    nocontext.mkdir()
    for k, text in ((1, "a\t3\nb\t2\n"), (2, "a b\t2\n"), (3, "a b a\t1\nb a b\t1\n")):
        (nocontext / ("%d-gm" % k)).write_text(text)
    _refused(LanguageModel(str(nocontext), 3, "<S>", "</S>", ("english",), id_order="lines"), out, 3)
    unknown = tmp_path / "unknown"                                               # "zz" is no word: the entry ends in the unknown id
    unknown.mkdir()
    for k, text in ((1, "a\t3\nb\t2\n"), (2, "a b\t2\na zz\t1\n")):
        (unknown / ("%d-gm" % k)).write_text(text)
    _refused(LanguageModel(str(unknown), 2, "<S>", "</S>", ("english",), id_order="lines"), out, 2)


def test_unwritable_directory_is_an_invalid_argument(tmp_path):
    from suggest_amd import _lib
    from suggest_amd.spell import LanguageModel
    src = LanguageModel(LM_DIR, id_order="count")
    missing = tmp_path / "no" / "such" / "dir"
    with pytest.raises(_lib.SuggestHipError) as e:
        src.save_ngrams(missing, device=-1)
    assert e.value.code == SG_E_INVALID and str(missing / "1-gm") in str(e.value)
    L = _lib.lib()
    assert L.sg_lm_store_google(None, b"x", -1) == SG_E_INVALID
    assert L.sg_lm_store_google(src._h, None, -1) == SG_E_INVALID
    assert L.sg_debug_lm_store_times(None) == SG_E_INVALID
    assert L.sg_debug_lm_store_slice_bytes(4096) == 0 and L.sg_debug_lm_store_slice_bytes(0) == 0


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """mph_build and the host writer compiled with -fsanitize=address,undefined into a program of their own"""
    r = subprocess.run([cpp_program(), LM_DIR, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr


def test_go_shim_and_cpp_mirror_follow_the_header(tmp_path):
    """go/suggesthip/suggesthip.go has never met a Go compiler: the new calls pass as many arguments as the header declares;
    the C++ mirror's pair compiles"""
    go = open(os.path.join(ROOT, "go", "suggesthip", "suggesthip.go"), encoding="utf-8").read()
    header = open(os.path.join(ROOT, "include", "suggest_hip.h"), encoding="utf-8").read()
    for fn in ("sg_lm_store_binary_ex", "sg_lm_store_google"):
        decl = re.search(r"int %s\(([^;]*)\);" % fn, header).group(1)
        call = re.search(r"C\.%s\(([^\n]*)\)\n" % fn, go)
        assert call, fn
        assert call.group(1).count(",") == decl.count(","), fn
    assert "func (s *SpellChecker) StoreBinary(lmPath, cdbPath string, mph bool) error" in go
    assert "func (s *SpellChecker) StoreNGrams(dir string, device int) error" in go
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "suggest_hip.hpp"\nvoid f(const suggest::lm::LanguageModel& m) { m.StoreBinary("a.lm", "a.cdb", true); m.StoreNGrams("d"); m.StoreNGrams("d", 0); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
