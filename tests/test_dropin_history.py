"""The history / inter-matrix / AEDataset mirror on the host: what `dropin.install(history=True)` rebinds and what
`install()` leaves alone, the signatures, the assertion and the errors raised before a device is asked for, the refusal to
run without a device and the argument checks of daisy_history_* (before any HIP call)."""
import ctypes
import inspect
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

host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="host-only check (with a device the call would run)")

MODEL_MODULES = ("MFRecommender", "FMRecommender", "NeuMFRecommender", "Item2VecRecommender", "LightGCNRecommender",
                 "NGCFRecommender", "NFMRecommender", "VAECFRecommender", "SLiMRecommender", "PureSVDRecommender",
                 "EASERecommender", "KNNCFRecommender", "PopRecommender")

CHECK = """
import sys
sys.path[:0] = %r
import daisy.utils.utils as u
import daisy.utils.dataset as ds
before = {(m.__name__, k): getattr(m, k) for m in (u, ds) for k in dir(m) if not k.startswith('__')}
import daisyrec_amd.dropin as d
import daisyrec_amd.utils.utils as U
import daisyrec_amd.utils.dataset as D
d.install()
assert all(getattr(sys.modules[m], k) is v for (m, k), v in before.items()), 'install() touched utils / dataset'
d.install(front_end=True)
assert u.get_history_matrix is before[('daisy.utils.utils', 'get_history_matrix')], 'front_end rebinds the history names'
assert ds.AEDataset is before[('daisy.utils.dataset', 'AEDataset')]
d.install(history=True)
assert tuple(d.HISTORY_NAMES) == ('get_history_matrix', 'get_inter_matrix')
assert u.get_history_matrix is U.get_history_matrix and u.get_inter_matrix is U.get_inter_matrix
assert ds.AEDataset is D.AEDataset
changed = sorted(k for (m, k), v in before.items() if getattr(sys.modules[m], k) is not v)
assert changed == ['AEDataset', 'build_candidates_set', 'get_history_matrix', 'get_inter_matrix', 'get_ir', 'get_ur'], changed
"""


def _run(paths):
    r = subprocess.run([sys.executable, "-c", CHECK % (list(paths),)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_install_rebinds_history_only_on_request(tmp_path):
    """against a stand-in `daisy` package that only has the modules install() touches: needs no reference checkout"""
    pkg = tmp_path / "daisy"
    for sub in ("model", "utils"):
        (pkg / sub).mkdir(parents=True)
        (pkg / sub / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("")
    for name in MODEL_MODULES:
        (pkg / "model" / f"{name}.py").write_text("")
    for name in ("sampler", "metrics", "loader", "splitter"):
        (pkg / "utils" / f"{name}.py").write_text("")
    (pkg / "utils" / "utils.py").write_text(
        "def get_ur(df):\n    return 'reference'\ndef get_ir(df):\n    return 'reference'\n"
        "def build_candidates_set(*a):\n    return 'reference'\ndef get_history_matrix(*a):\n    return 'reference'\n"
        "def get_inter_matrix(*a):\n    return 'reference'\ndef ensure_dir(p):\n    return 'reference'\n")
    (pkg / "utils" / "dataset.py").write_text(
        "class BasicDataset(object):\n    pass\nclass CandidatesDataset(object):\n    pass\nclass AEDataset(object):\n    pass\n"
        "def get_dataloader(*a):\n    return 'reference'\n")
    _run([str(tmp_path), ROOT])


def test_install_rebinds_the_reference_checkout():
    if not os.path.isdir(os.path.join(REF, "daisy")):
        pytest.skip("reference checkout not present")
    _run([os.path.join(ROOT, "tests", "golden", "_shims"), REF, ROOT])


def test_signatures_equal_the_reference():
    from daisyrec_amd.utils import dataset as D, utils as U
    want = {"get_history_matrix": "(df, config, row='user', use_config_value_name=False)",
            "get_inter_matrix": "(df, config, form='coo')"}
    for name, sig in want.items():
        assert str(inspect.signature(getattr(U, name))) == sig
    assert str(inspect.signature(U.history_csr)) == want["get_history_matrix"]
    assert str(inspect.signature(D.AEDataset.__init__)) == "(self, train_set, yield_col='user')"
    if not os.path.isdir(os.path.join(REF, "daisy")):
        return
    code = ("import sys, inspect\n"
            f"sys.path[:0] = {[os.path.join(ROOT, 'tests', 'golden', '_shims'), REF]!r}\n"
            "import daisy.utils.utils as u, daisy.utils.dataset as d\n"
            "print(inspect.signature(u.get_history_matrix)); print(inspect.signature(u.get_inter_matrix))\n"
            "print(inspect.signature(d.AEDataset.__init__))\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split("\n")[:3] == [want["get_history_matrix"], want["get_inter_matrix"], "(self, train_set, yield_col='user')"]


# ---- errors raised on the host, before a device is needed ----------------------------------------------------------------
def _config(**over):
    cfg = {"UID_NAME": "user", "IID_NAME": "item", "INTER_NAME": "rating", "user_num": 5, "item_num": 4,
           "logger": logging.getLogger("test")}
    cfg.update(over)
    return cfg


def _frame(**over):
    cols = {"user": [3, 0, 3, 1, 0, 3, 1], "item": [0, 0, 2, 0, 1, 0, 3], "rating": [5, 4, 0, 2, 3, 1, 2.5]}
    cols.update(over)
    return pd.DataFrame(cols)


def test_errors_before_a_device_is_needed():
    from daisyrec_amd.utils import utils as U
    for fn in (U.get_history_matrix, U.history_csr):
        with pytest.raises(AssertionError, match="invalid name users: not in columns of history dataframe"):
            fn(_frame(), _config(), row="users")
        with pytest.raises(IndexError, match="index 5 is out of bounds"):
            fn(_frame(user=[3, 0, 5, 1, 0, 3, 1]), _config())
        with pytest.raises(IndexError, match="index 4 is out of bounds"):
            fn(_frame(item=[0, 0, 2, 0, 4, 0, 3]), _config())
        with pytest.raises(IndexError, match="index -1 is out of bounds"):          # numpy would wrap it
            fn(_frame(item=[0, 0, 2, 0, -1, 0, 3]), _config())
        with pytest.raises(IndexError, match="index 4 is out of bounds"):           # row='item': the items are the rows
            fn(_frame(item=[0, 0, 2, 0, 4, 0, 3]), _config(), row="item")
        with pytest.raises(KeyError):
            fn(_frame(), {k: v for k, v in _config().items() if k != "logger"} if fn is U.get_history_matrix else
               {k: v for k, v in _config().items() if k != "user_num"})
    with pytest.raises(NotImplementedError, match=r"Sparse matrix format \[csc\] has not been implemented..."):
        U.get_inter_matrix(_frame(), _config(), form="csc")
    with pytest.raises(IndexError, match="index 7 is out of bounds"):
        U.get_inter_matrix(_frame(user=[3, 0, 7, 1, 0, 3, 1]), _config())


@host_only
def test_no_cpu_path():
    from daisyrec_amd.utils import utils as U
    from daisyrec_amd.utils.dataset import AEDataset
    for call, name in ((lambda: U.get_history_matrix(_frame(), _config()), "get_history_matrix"),
                       (lambda: U.get_history_matrix(_frame(), _config(), row="item", use_config_value_name=True),
                        "get_history_matrix"),
                       (lambda: U.history_csr(_frame(), _config()), "history_csr"),
                       (lambda: U.get_inter_matrix(_frame(), _config()), "get_inter_matrix"),
                       (lambda: U.get_inter_matrix(_frame(), _config(), "csr"), "get_inter_matrix"),
                       (lambda: AEDataset(_frame()), "AEDataset"),
                       (lambda: AEDataset(_frame(), yield_col="item"), "AEDataset")):
        with pytest.raises(RuntimeError, match=f"daisyrec_amd.{name} needs a HIP device"):
            call()


def test_device_inter_matrix_surface_needs_no_device():
    """the object itself is plain bookkeeping: host tensors show its interface"""
    from daisyrec_amd.utils.utils import DeviceInterMatrix
    m = DeviceInterMatrix(torch.tensor([3, 0, 3], dtype=torch.int32), torch.tensor([0, 0, 2], dtype=torch.int32),
                          torch.tensor([5.0, 4.0, 0.0], dtype=torch.float64), (5, 4))
    assert m.shape == (5, 4) and m.nnz == 3 and m.tocoo() is m and m.format == "coo"
    sp = pytest.importorskip("scipy.sparse")
    s = m.to_scipy()
    assert sp.isspmatrix_coo(s) and s.shape == (5, 4) and s.nnz == 3 and s.row.dtype == np.int32 and s.data.dtype == np.float64
    assert s.row.tolist() == [3, 0, 3] and s.col.tolist() == [0, 0, 2] and s.data.tolist() == [5.0, 4.0, 0.0]


def test_vaecf_checks_a_given_csr_without_a_device():
    """config['history_csr']: the padded pair may be absent; what is wrong with the CSR is said before a kernel reads it"""
    from daisyrec_amd.model.VAECFRecommender import VAECF
    cfg = {"gpu": "0", "epochs": 1, "lr": 0.01, "dropout": 0.5, "mlp_hidden_size": [8], "latent_dim": 4, "anneal_cap": 0.2,
           "total_anneal_steps": 10, "user_num": 5, "item_num": 4, "optimizer": "default", "init_method": "default",
           "early_stop": False, "topk": 2, "history_item_id": None, "history_item_value": None}
    good = (torch.tensor([0, 1, 2, 2, 3, 3]), torch.tensor([1, 3, 0], dtype=torch.int32), torch.tensor([3.0, 2.5, 1.0]), 3)
    m = VAECF(dict(cfg, history_csr=good))
    assert m.history_item_id is None and m.history_item_value is None
    if m.device == "cpu":
        row_ptr, col, val = m._checked_csr(good)
        assert row_ptr.tolist() == [0, 1, 2, 2, 3, 3] and col.dtype == torch.int32 and val.dtype == torch.float32
        m._check_users(torch.tensor([0, 4]))
        with pytest.raises(IndexError, match="index 5 is out of bounds for dimension 0 with size 5"):
            m._check_users(torch.tensor([5]))
        bad = [((good[0][:-1], good[1], good[2]), ValueError, "row_ptr"),
               ((good[0].to(torch.int32), good[1], good[2]), TypeError, "int64 / int32 / float32"),
               ((good[0], good[1].long(), good[2]), TypeError, "int64 / int32 / float32"),
               ((good[0], good[1], good[2][:2]), ValueError, "col / val"),
               ((torch.tensor([0, 1, 2, 2, 3, 2]), good[1], good[2]), ValueError, "ascend from 0 to nnz = 3"),
               ((good[0], torch.tensor([1, 4, 0], dtype=torch.int32), good[2]), IndexError, r"\[0, 4\)"),
               ((good[0], good[1]), TypeError, "expected")]
        for given, exc, text in bad:
            with pytest.raises(exc, match=text):
                m._checked_csr(given)
    with pytest.raises((KeyError, AttributeError)):            # without the key the padded pair is required, as before
        VAECF({k: v for k, v in cfg.items() if k != "history_item_id"})


# ---- DAISY_ERR_ARG: before any HIP call (the pointers are dummies nobody reads) ------------------------------------------
def test_native_argument_errors_need_no_device():
    from daisyrec_amd import _native as N
    buf = ctypes.create_string_buffer(256)
    d = ctypes.addressof(buf)
    one = (ctypes.c_int64 * 2)()
    L = N.lib

    def counts(row=d, n=10, row_num=3, order=d, longest=one):
        return L.daisy_history_counts(row, n, row_num, order, d, d, longest, None)

    def fill(order=d, val=None, n=10, row_num=3, width=4, out=d):
        return L.daisy_history_fill(order, d, d, val, n, row_num, width, out, d, None)

    def csr(row=d, val=None, n=10, row_num=3, col_num=4, totals=one):
        return L.daisy_history_csr(row, d, val, n, row_num, col_num, d, d, d, totals, None)

    def first(ids=d, n=10, id_num=3, count=one):
        return L.daisy_history_first_seen(ids, n, id_num, d, count, None)

    cases = [(lambda: counts(row=None), "history_counts: NULL argument"), (lambda: counts(order=None), "history_counts: NULL"),
             (lambda: counts(longest=None), "history_counts: NULL argument"),
             (lambda: counts(n=0), "history_counts: n=0 outside [1, 2^31)"), (lambda: counts(n=2 ** 31), "outside [1, 2^31)"),
             (lambda: counts(row_num=0), "history_counts: row_num=0 outside"), (lambda: counts(row_num=2 ** 31), "row_num="),
             (lambda: fill(order=None), "history_fill: NULL argument"), (lambda: fill(out=None), "history_fill: NULL argument"),
             (lambda: fill(n=0), "history_fill: n=0 outside"), (lambda: fill(n=2 ** 31), "outside [1, 2^31)"),
             (lambda: fill(row_num=0), "history_fill: row_num=0"), (lambda: fill(width=0), "history_fill: L=0 outside [1, n]"),
             (lambda: fill(width=11), "history_fill: L=11 outside [1, n]"),
             (lambda: csr(row=None), "history_csr: NULL argument"), (lambda: csr(totals=None), "history_csr: NULL argument"),
             (lambda: csr(n=0), "history_csr: n=0 outside"), (lambda: csr(n=2 ** 31), "outside [1, 2^31)"),
             (lambda: csr(row_num=0), "history_csr: row_num=0"), (lambda: csr(col_num=0), "history_csr: col_num=0"),
             (lambda: csr(col_num=2 ** 31), "history_csr: col_num="),
             (lambda: first(ids=None), "history_first_seen: NULL argument"), (lambda: first(count=None), "history_first_seen: NULL"),
             (lambda: first(n=0), "history_first_seen: n=0 outside"), (lambda: first(n=2 ** 31), "outside [1, 2^31)"),
             (lambda: first(id_num=0), "history_first_seen: id_num=0")]
    for call, text in cases:
        rc = call()
        assert rc == N.DAISY_ERR_ARG, (text, rc)
        assert text in N.last_error(), (text, N.last_error())
        with pytest.raises(ValueError):
            N.check(rc)


@host_only
def test_unmodified_driver_reaches_the_device_history(tmp_path):
    """run_examples/test.py of the reference checkout, unmodified, with --algo_name multi-vae under install(history=True):
    it gets as far as get_history_matrix and stops there with the no-device error."""
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
            "d.install(history=True)\n"
            "sys.argv = ['test.py', '--algo_name', 'multi-vae', '--dataset', 'ml-100k', '--prepro', 'origin']\n"
            f"runpy.run_path({os.path.join(REF, 'run_examples', 'test.py')!r}, run_name='__main__')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode != 0
    assert "daisyrec_amd.get_history_matrix needs a HIP device" in r.stderr, r.stderr[-3000:]
