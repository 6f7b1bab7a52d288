"""The Preprocessor / splitter mirror on the host: what `dropin.install(prep=True)` rebinds and what `install()` leaves
alone, the `ValueError` / `TypeError`s (raised before a device is asked for), the refusal to run without a device, the
host-side splits (tsbr, cv) and the argument checks of daisy_prep_* / daisy_split_ids (before any HIP call)."""
import ctypes
import logging
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DAISY_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prep_oracle as O  # noqa: E402

host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="host-only check (with a device the call would run)")

MODEL_MODULES = ("MFRecommender", "FMRecommender", "NeuMFRecommender", "Item2VecRecommender", "LightGCNRecommender",
                 "NGCFRecommender", "NFMRecommender", "VAECFRecommender", "SLiMRecommender", "PureSVDRecommender",
                 "EASERecommender", "KNNCFRecommender", "PopRecommender")

CHECK = """
import sys
sys.path[:0] = %r
import daisy.utils.loader as l
import daisy.utils.splitter as s
before = {(m.__name__, k): getattr(m, k) for m in (l, s) for k in dir(m) if not k.startswith('__')}
import daisyrec_amd.dropin as d
import daisyrec_amd.utils.loader as L
import daisyrec_amd.utils.splitter as S
d.install()
assert all(getattr(sys.modules[m], k) is v for (m, k), v in before.items()), 'install() touched loader / splitter'
d.install(prep=True)
assert l.Preprocessor is L.Preprocessor
names = ('TestSplitter', 'ValidationSplitter', 'split_test', 'split_validation')
assert tuple(d.SPLITTER_NAMES) == names
for k in names:
    assert getattr(s, k) is getattr(S, k), k
assert l.RawDataReader is before[('daisy.utils.loader', 'RawDataReader')]
"""


def _run(paths):
    r = subprocess.run([sys.executable, "-c", CHECK % (list(paths),)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_install_rebinds_prep_only_on_request(tmp_path):
    """against a stand-in `daisy` package that only has the modules install() touches: needs no reference checkout"""
    pkg = tmp_path / "daisy"
    for sub in ("model", "utils"):
        (pkg / sub).mkdir(parents=True)
        (pkg / sub / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("")
    for name in MODEL_MODULES:
        (pkg / "model" / f"{name}.py").write_text("")
    for name in ("sampler", "utils", "metrics"):
        (pkg / "utils" / f"{name}.py").write_text("")
    (pkg / "utils" / "loader.py").write_text("class RawDataReader(object):\n    pass\nclass Preprocessor(object):\n    pass\n")
    (pkg / "utils" / "splitter.py").write_text(
        "class TestSplitter(object):\n    pass\nclass ValidationSplitter(object):\n    pass\n"
        "def split_test(*a):\n    return 'reference'\ndef split_validation(*a):\n    return 'reference'\n")
    _run([str(tmp_path), ROOT])


def test_install_rebinds_the_reference_checkout():
    if not os.path.isdir(os.path.join(REF, "daisy")):
        pytest.skip("reference checkout not present")
    _run([os.path.join(ROOT, "tests", "golden", "_shims"), REF, ROOT])


# ---- errors raised on the host, before a device is needed ----------------------------------------------------------------
def _config(**over):
    cfg = {"dataset": "t", "prepro": "3core", "UID_NAME": "user", "IID_NAME": "item", "TID_NAME": "timestamp",
           "INTER_NAME": "rating", "binary_inter": True, "positive_threshold": None, "level": "ui",
           "logger": logging.getLogger("test"), "metrics": ["ndcg", "popularity"]}
    cfg.update(over)
    return cfg


def _frame(**over):
    cols = {"user": [1, 1, 2], "item": [5, 6, 5], "rating": [1.0, 2.0, 3.0], "timestamp": [3, 2, 1]}
    cols.update(over)
    return pd.DataFrame(cols)


def test_preprocessor_surface_and_errors_need_no_device():
    from daisyrec_amd.utils.loader import Preprocessor, _codes_dtype
    p = Preprocessor(_config())
    assert (p.user_num, p.item_num, p.item_pop, p.get_pop) == (None, None, None, True)
    assert p.get_user_num() is None and p.get_item_num() is None
    assert not Preprocessor(_config(metrics=["ndcg"])).get_pop
    with pytest.raises(ValueError, match="origin/Ncore/Nfilter"):
        Preprocessor(_config(prepro="5kernel")).process(_frame())
    with pytest.raises(ValueError, match="origin/Ncore/Nfilter"):
        Preprocessor(_config(prepro="core")).process(_frame())
    with pytest.raises(ValueError, match="Invalid level value: iu"):
        Preprocessor(_config(level="iu")).process(_frame())
    with pytest.raises(ValueError, match="N must be >= 1"):
        Preprocessor(_config(prepro="0core")).process(_frame())
    with pytest.raises(TypeError, match="float64"):
        Preprocessor(_config()).process(_frame(timestamp=[1.0, 2.0, 3.5]))
    with pytest.raises(TypeError, match="object"):
        Preprocessor(_config()).process(_frame(timestamp=["a", "b", "c"]))
    # pd.Categorical(...).codes: int8 up to 126 categories, int16 up to 32766, then int32
    assert [np.dtype(_codes_dtype(k)).name for k in (0, 126, 127, 128, 32766, 32767, 2 ** 31 - 2, 2 ** 31 - 1)] == [
        "int8", "int8", "int16", "int16", "int16", "int32", "int32", "int64"]
    for k in (1, 126, 127, 128):
        assert pd.Categorical(np.arange(k)).codes.dtype == _codes_dtype(k)


def test_splitter_errors_and_host_splits_need_no_device():
    from daisyrec_amd.utils import splitter as S
    df = _frame()
    with pytest.raises(ValueError, match="Invalid data_split value"):
        S.split_test(df, "loo")
    with pytest.raises(ValueError, match="Invalid val_method"):
        S.split_validation(df, "loo")
    for size in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="outside"):
            S.split_test(df, "ufo", size)
        with pytest.raises(ValueError, match="outside"):
            S.split_test(df, "tsbr", size)
    with pytest.raises(TypeError, match="float64"):
        S.split_test(_frame(timestamp=[1.0, 2.0, 3.5]), "tloo")
    with pytest.raises(ValueError, match="fold_num"):
        S.split_validation(df, "cv", 1)
    assert S.TestSplitter({"test_method": "tsbr", "test_size": 0.2, "UID_NAME": "user", "TID_NAME": "timestamp"}).seed == 2022
    cfg = {"val_method": "cv", "fold_num": 3, "val_size": 0.1, "UID_NAME": "user", "TID_NAME": "timestamp", "seed": 7}
    assert S.ValidationSplitter(cfg).seed == 7
    # tsbr and cv are index arithmetic on the host
    for n, size in O.TSBR_CASES:
        frame = pd.DataFrame({"user": np.zeros(n, dtype=np.int64)})
        for got in (S.split_test(frame, "tsbr", size), next(iter(S.split_validation(frame, "tsbr", 1, size)))):
            want = O.split_tsbr(n, size)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for n, k in O.CV_CASES:
        frame = pd.DataFrame({"user": np.zeros(n, dtype=np.int64)})
        cfg["fold_num"] = k
        folds = list(S.ValidationSplitter(cfg).split(frame))
        assert len(folds) == k
        for (tr, va), (wtr, wva) in zip(folds, O.split_cv(n, k)):
            assert np.array_equal(tr, wtr) and np.array_equal(va, wva) and tr.dtype == np.int64


@host_only
def test_no_cpu_path():
    from daisyrec_amd.utils import splitter as S
    from daisyrec_amd.utils.loader import Preprocessor
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        Preprocessor(_config()).process(_frame())
    for method in ("tloo", "utfo", "ufo", "rloo", "rsbr"):
        with pytest.raises(RuntimeError, match="needs a HIP device"):
            S.split_test(_frame(), method, 0.5)
        with pytest.raises(RuntimeError, match="needs a HIP device"):
            list(S.split_validation(_frame(), method, 2, 0.5))


# ---- DAISY_ERR_ARG: before any HIP call (the pointers are dummies nobody reads) ------------------------------------------
def test_native_argument_errors_need_no_device():
    from daisyrec_amd import _native as N
    buf = ctypes.create_string_buffer(256)
    d = ctypes.addressof(buf)
    one = (ctypes.c_int64 * 4)()

    def process(users=d, rating=d, n=10, use_thr=0, mode=2, level=3, Nmin=5, want_pop=0, pop=None, stats=one):
        return N.lib.daisy_prep_process(users, d, rating, d, n, use_thr, 3.0, mode, level, Nmin, want_pop, d, d, d, d, d, pop,
                                        stats, None)

    def split(method=0, users=d, ts=d, n=10, user_num=3, size=0.2, train=d, counts=one):
        return N.lib.daisy_split_ids(method, users, ts, n, user_num, size, 1 - size, 1, 0, train, d, counts, None)

    cases = [(lambda: process(users=None), "NULL argument"), (lambda: process(stats=None), "NULL argument"),
             (lambda: process(use_thr=1, rating=None), "a threshold needs the ratings"),
             (lambda: process(want_pop=1), "NULL argument (item_pop)"),
             (lambda: process(n=0), "n=0 outside [1, 2^31)"), (lambda: process(n=2 ** 31), "outside [1, 2^31)"),
             (lambda: process(mode=3), "mode=3"), (lambda: process(level=0), "level=0"), (lambda: process(level=4), "level=4"),
             (lambda: process(Nmin=0), "N=0, must be >= 1"),
             (lambda: N.lib.daisy_prep_encode(None, 5, d, d, one, None), "NULL argument"),
             (lambda: N.lib.daisy_prep_encode(d, 5, d, d, None, None), "NULL argument"),
             (lambda: N.lib.daisy_prep_encode(d, 0, d, d, one, None), "n=0 outside"),
             (lambda: N.lib.daisy_prep_encode(d, 2 ** 31, d, d, one, None), "outside [1, 2^31)"),
             (lambda: split(method=5), "method=5"), (lambda: split(method=-1), "method=-1"),
             (lambda: split(train=None), "NULL argument"), (lambda: split(counts=None), "NULL argument"),
             (lambda: split(method=1, users=None), "NULL argument (user_code)"),
             (lambda: split(method=0, ts=None), "tloo needs the timestamps"),
             (lambda: split(n=0), "n=0 outside"), (lambda: split(n=2 ** 31), "outside [1, 2^31)"),
             (lambda: split(user_num=0), "user_num=0"), (lambda: split(user_num=11), "user_num=11"),
             (lambda: split(method=1, size=0.0), "size=0 outside (0, 1)"), (lambda: split(method=2, size=1.0), "size=1 outside"),
             (lambda: split(method=4, size=-0.5), "outside (0, 1)"), (lambda: split(method=4, size=float("nan")), "outside (0, 1)")]
    for call, text in cases:
        rc = call()
        assert rc == N.DAISY_ERR_ARG, (text, rc)
        assert text in N.last_error(), (text, N.last_error())
        with pytest.raises(ValueError):
            N.check(rc)


@host_only
def test_unmodified_driver_reaches_the_device_preprocessor(tmp_path):
    """run_examples/test.py of the reference checkout, unmodified, under install(prep=True): it gets as far as
    processor.process and stops there with the no-device error."""
    if not os.path.isfile(os.path.join(REF, "run_examples", "test.py")):
        pytest.skip("reference checkout not present")
    data = tmp_path / "data" / "ml-100k"
    data.mkdir(parents=True)
    rng = np.random.default_rng(0)
    rows = np.stack([rng.integers(1, 30, 400), rng.integers(1, 40, 400), rng.integers(1, 6, 400), rng.permutation(400)], 1)
    np.savetxt(data / "u.data", rows, fmt="%d", delimiter="\t")
    code = ("import sys, os, runpy\n"
            f"sys.path[:0] = {[os.path.join(ROOT, 'tests', 'golden', '_shims'), REF, ROOT]!r}\n"
            "import daisyrec_amd.dropin as d\n"
            "d.install(prep=True)\n"
            "sys.argv = ['test.py', '--algo_name', 'mostpop', '--dataset', 'ml-100k', '--prepro', '2core']\n"
            f"runpy.run_path({os.path.join(REF, 'run_examples', 'test.py')!r}, run_name='__main__')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode != 0
    assert "daisyrec_amd.Preprocessor.process needs a HIP device" in r.stderr, r.stderr[-3000:]
