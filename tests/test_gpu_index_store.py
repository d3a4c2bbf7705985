"""sg_index_store_reference with the device encoder (index_store.inc): the checks of tests/test_index_store_cpu.py on the bytes
the kernels write — against the reference's own files under golden/db, the Python encoders and the host encoder's files — and
that a save leaves the search path of the same device alone."""
import os
import subprocess

import numpy as np
import pytest

import refindex
from conftest import CARS_DESC, WORDS_DESC
from index_store_shapes import check_saved, check_shapes, cpp_program, dropped_repeats_files, fixture_lists, type_prefix

pytestmark = pytest.mark.gpu


def _desc(d):
    from suggest_amd import IndexDescription
    return IndexDescription(**d)


def _save(ix, tmp_path, name, device):
    hd, dl = str(tmp_path / (name + ".hd")), str(tmp_path / (name + ".dl"))
    ix.save(hd, dl, device=device)
    return hd, dl


def _same_files(a, b):
    for x, y in zip(a, b):
        assert open(x, "rb").read() == open(y, "rb").read(), (x, y)


def test_cars_encoded_on_the_device(cars_lines, tmp_path, golden_dir):
    from suggest_amd import NGramIndex
    ix = NGramIndex(cars_lines, _desc(CARS_DESC), upload=False)
    hd, dl = _save(ix, tmp_path, "cars", 0)
    assert os.path.getsize(dl) == 154469
    indices, terms = check_saved(hd, dl, fixture_lists(golden_dir, "cars"))
    assert indices == 52 and len(terms) == 36285
    _, _, ref_terms = refindex.read_header(os.path.join(golden_dir, "db", "cars.hd"))
    assert {(t, i, s, n) for t, i, s, _, n in terms} == {(t, i, s, n) for t, i, s, _, n in ref_terms}
    assert sum(1 for t in terms if t[4] <= 65) == 36276 and sum(1 for t in terms if 65 < t[4] <= 256) == 9
    assert type_prefix(open(hd, "rb").read()) == type_prefix(open(os.path.join(golden_dir, "db", "cars.hd"), "rb").read())
    _same_files((hd, dl), _save(ix, tmp_path, "cars_host", -1))
    assert NGramIndex.from_reference_files(hd, dl, _desc(CARS_DESC), upload=False).lists() == ix.lists()


def test_edge_shapes_encoded_on_the_device(tmp_path, golden_dir):
    check_shapes(tmp_path, golden_dir, 0)


def test_dropped_repeats_encoded_on_the_device(tmp_path, golden_dir):
    from suggest_amd import NGramIndex
    desc, hd, dl = dropped_repeats_files(tmp_path, golden_dir)
    ix = NGramIndex.from_reference_files(hd, dl, _desc(desc), upload=False)
    saved = _save(ix, tmp_path, "t_dev", 0)
    _same_files(saved, _save(ix, tmp_path, "t_host", -1))
    assert NGramIndex.from_reference_files(saved[0], saved[1], _desc(desc), upload=False).lists() == ix.lists()


def test_words_encoded_on_the_device(words_lines, tmp_path, golden_dir):
    from suggest_amd import NGramIndex
    ix = NGramIndex(words_lines, _desc(WORDS_DESC), upload=False)
    hd, dl = _save(ix, tmp_path, "words", 0)
    want = fixture_lists(golden_dir, "words_subset")
    assert len(want) == 7311 and sum(1 for raw, _ in want.values() if raw > 256) == 40
    check_saved(hd, dl, want)
    _same_files((hd, dl), _save(ix, tmp_path, "words_host", -1))


def test_device_built_index_saved_on_the_device(cars_lines, tmp_path):
    from suggest_amd import NGramIndex, synth
    blob, offs = synth.make_dict(30000, seed=5)
    for name, kw, d in (("cars", dict(docs=cars_lines), _desc(CARS_DESC)), ("synth", dict(blob=blob, offs=offs), _desc(synth.DESCRIPTION))):
        dev = NGramIndex(description=d, device=0, upload=False, build="device", **kw)
        host = NGramIndex(description=d, upload=False, build="host", **kw)
        first = _save(dev, tmp_path, name + "_dev", None)             # device=None: the GPU that built it
        _same_files(first, _save(host, tmp_path, name + "_host", -1))
        _same_files(first, _save(dev, tmp_path, name + "_dev_again", 0))


def test_save_leaves_the_search_path_alone(cars_lines, tmp_path):
    from suggest_amd import NGramIndex, pack_strings
    queries = [l[:-1] if i % 3 == 0 and len(l) > 4 else l for i, l in enumerate(cars_lines[::25][:200])]
    assert len(queries) == 200
    qb, qo = pack_strings(queries)
    ix = NGramIndex(cars_lines, _desc(CARS_DESC), device=0)

    def rows(index):
        out = []
        for metric, alpha, k in (("jaccard", 0.4, 10), ("cosine", 0.5, 7)):
            out.extend(index.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=k))
        out.extend(index.autocomplete_batch(blob=qb, offs=qo, limit=10))
        return out

    def same(a, b):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))

    before = rows(ix)
    assert int(before[2].sum()) > 0
    hd, dl = _save(ix, tmp_path, "cars", None)                        # device=None: the index's own GPU
    same(rows(ix), before)
    assert ix.replicas() == [0]
    same(rows(NGramIndex.from_reference_files(hd, dl, _desc(CARS_DESC), device=0)), before)


def test_cpp_mirror_indexes_cars_on_the_device(tmp_path, golden_dir):
    r = subprocess.run([cpp_program(), golden_dir, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
    check_saved(str(tmp_path / "cars.hd"), str(tmp_path / "cars.dl"), fixture_lists(golden_dir, "cars"))
