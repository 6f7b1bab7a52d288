"""The KPI mirror and MostPop on the host: what `dropin.install(metrics=True)` rebinds and what `install()` leaves alone, the
`ValueError`s of daisyrec_amd.utils.metrics and MostPop (raised before a device is asked for), the refusal to run without
a device, and the argument checks of daisy_ranking_kpis / daisy_pop_* (before any HIP call)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
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
import daisy.utils.metrics as m
before = {k: getattr(m, k) for k in dir(m) if not k.startswith('__')}
import daisyrec_amd.dropin as d
import daisyrec_amd.utils.metrics as M
from daisyrec_amd.model import MostPop
d.install()
import daisy.model.PopRecommender as p
assert p.MostPop is MostPop
assert all(getattr(m, k) is v for k, v in before.items()), 'install() touched daisy.utils.metrics'
d.install(metrics=True)
names = ('metrics_name_config', 'calc_ranking_results', 'Metric', 'Coverage', 'Popularity', 'Diversity', 'Precision', 'Recall',
         'MRR', 'MAP', 'NDCG', 'HR', 'AUC', 'F1')
assert tuple(d.METRICS_NAMES) == names
for k in names:
    assert getattr(m, k) is getattr(M, k), k
assert m.metrics_name_config['map'] == 'MAP'
"""


def _run(paths):
    r = subprocess.run([sys.executable, "-c", CHECK % (list(paths),)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_install_rebinds_the_metrics_only_on_request(tmp_path):
    """against a stand-in `daisy` package that only has the modules install() touches: needs no reference checkout"""
    pkg = tmp_path / "daisy"
    for sub in ("model", "utils"):
        (pkg / sub).mkdir(parents=True)
        (pkg / sub / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("")
    for name in MODEL_MODULES:
        (pkg / "model" / f"{name}.py").write_text("")
    for name in ("sampler", "utils"):
        (pkg / "utils" / f"{name}.py").write_text("")
    (pkg / "utils" / "metrics.py").write_text(
        "metrics_name_config = {}\n" + "".join(f"def {f}(*a):\n    return 'reference'\n" for f in (
            "calc_ranking_results", "Coverage", "Popularity", "Diversity", "Precision", "Recall", "MRR", "MAP", "NDCG", "HR",
            "AUC", "F1")) + "class Metric(object):\n    pass\n")
    _run([str(tmp_path), ROOT])


def test_install_rebinds_the_reference_checkout():
    if not os.path.isdir(os.path.join(REF, "daisy")):
        pytest.skip("reference checkout not present")
    _run([os.path.join(ROOT, "tests", "golden", "_shims"), REF, ROOT])


# ---- ValueErrors: raised on the host, before a device is needed --------------------------------------------------------
def _kpis(**over):
    from daisyrec_amd.utils import metrics as M
    args = dict(pred=np.array([[1, 2, 3], [0, 4, 2]]), gt_csr_or_test_ur={0: {1}, 1: {4, 0}}, test_u=[0, 1], cutoffs=[1, 3],
                metrics=["precision"], item_num=5)
    args.update(over)
    return M.ranking_kpis(**args)


def test_value_errors_need_no_device():
    with pytest.raises(ValueError, match=r"item id 5 outside \[0, 5\)"):
        _kpis(pred=np.array([[1, 2, 5], [0, 4, 2]]))
    with pytest.raises(ValueError, match=r"item id -1 outside"):
        _kpis(pred=np.array([[1, -1, 3], [0, 4, 2]], dtype=np.int32))
    with pytest.raises(ValueError, match="non-integral"):
        _kpis(pred=np.array([[1, 2.5, 3], [0, 4, 2]], dtype=np.float32))
    with pytest.raises(ValueError, match="non-integral"):
        _kpis(pred=torch.tensor([[1, 2.5, 3], [0, 4, 2]]))
    with pytest.raises(ValueError, match="user 2 of test_u has no ground truth"):
        _kpis(test_u=[0, 2])
    with pytest.raises(ValueError, match="user 1 of test_u has no ground truth"):
        _kpis(gt_csr_or_test_ur={0: {1}, 1: set()})
    with pytest.raises(ValueError, match="0/1"):
        _kpis(metrics=["diversity"], i_categories=np.array([[0, 1], [2, 0], [0, 0], [1, 1], [1, 0]]))
    with pytest.raises(ValueError, match="needs i_categories"):
        _kpis(metrics=["diversity"])
    with pytest.raises(ValueError, match="needs item_pop"):
        _kpis(metrics=["popularity"])
    with pytest.raises(ValueError, match="Invalid metric name serendipity"):
        _kpis(metrics=["precision", "serendipity"])
    with pytest.raises(ValueError, match="2 users for 2 lists|1 users for 2 lists"):
        _kpis(test_u=[0])


def test_pack_categories_bits():
    from daisyrec_amd.utils.metrics import pack_categories
    cats = np.zeros((3, 65), dtype=np.int64)
    cats[0, 0] = cats[1, 63] = cats[2, 64] = cats[2, 1] = 1
    bits, C = pack_categories(cats)
    assert C == 65 and bits.dtype == np.int64 and bits.shape == (3, 2)
    assert bits.view(np.uint64).tolist() == [[1, 0], [1 << 63, 0], [2, 1]]


@host_only
def test_no_cpu_path():
    from daisyrec_amd.utils import metrics as M
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        _kpis()
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        M.Precision({0: {1}}, np.array([[1.0, 2.0]], dtype=np.float32), [0])
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        M.Coverage(np.array([[1, 2]]), 5)


def _pop_config(**over):
    cfg = {"gpu": "0", "item_num": 6, "topk": 3, "IID_NAME": "item"}
    cfg.update(over)
    return cfg


def test_mostpop_surface_errors_without_a_device():
    import pandas as pd
    from daisyrec_amd.model import MostPop
    m = MostPop(_pop_config())
    assert (m.item_num, m.topk, m.cnt_col) == (6, 3, "item")
    assert np.array_equal(m.item_cnt_ref, np.zeros(6)) and m.item_score is None
    with pytest.raises(ValueError, match="item_num=0"):
        MostPop(_pop_config(item_num=0))
    with pytest.raises(ValueError, match="topk=0"):
        MostPop(_pop_config(topk=0))
    with pytest.raises(ValueError, match=r"item id 6 outside \[0, 6\)"):
        m.fit(pd.DataFrame({"item": [1, 6, 2]}))
    with pytest.raises(ValueError, match=r"item id -1 outside"):
        m.fit(pd.DataFrame({"item": [1, -1, 2]}))
    with pytest.raises(ValueError, match="non-integer"):
        m.fit(pd.DataFrame({"item": [1.0, 2.5]}))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device visible"):
            m.fit(pd.DataFrame({"item": [1, 2, 2]}))
        with pytest.raises(RuntimeError, match="no HIP device visible"):
            m.full_rank(0)


# ---- DAISY_ERR_ARG: before any HIP call (the pointers are dummies nobody reads) ----------------------------------------
def test_native_argument_errors_need_no_device():
    from daisyrec_amd import _native as N
    buf = ctypes.create_string_buffer(256)
    d = ctypes.addressof(buf)
    cuts = lambda *ks: (ctypes.c_int32 * len(ks))(*ks)                                             # noqa: E731
    ALL = {k: 1 << v for k, v in N.KPI_IDS.items()}

    def call(pred=d, n=4, K=50, cutoffs=cuts(1, 5, 50), nc=3, disc=d, item_pop=None, cat=None, words=0, n_cats=0, sqrt_tab=None,
             metrics=ALL["precision"], means=d, cover=None, ws=d, ws_bytes=1 << 20, users=d):
        return N.lib.daisy_ranking_kpis(pred, 0, n, K, d, d, 10, users, cutoffs, nc, disc, item_pop, 100, cat, words, n_cats,
                                        sqrt_tab, metrics, None, means, cover, ws, ws_bytes, None)

    cases = [(dict(pred=None), "NULL argument"), (dict(users=None), "NULL argument"), (dict(cutoffs=None), "NULL argument"),
             (dict(means=None), "NULL argument (means)"),
             (dict(cutoffs=cuts(1, 5, 5)), "strictly ascending"), (dict(cutoffs=cuts(5, 1, 50)), "strictly ascending"),
             (dict(cutoffs=cuts(0, 5, 50)), "strictly ascending"), (dict(cutoffs=cuts(1, 5, 51)), "cutoff 51 exceeds K=50"),
             (dict(K=N.METRICS_MAX_K + 1), f"K={N.METRICS_MAX_K + 1} outside [1, {N.METRICS_MAX_K}]"),
             (dict(nc=N.METRICS_MAX_CUTOFFS + 1), "cutoffs outside"), (dict(n=0), "n=0"),
             (dict(metrics=ALL["popularity"]), "popularity needs its table"),
             (dict(metrics=ALL["diversity"]), "diversity needs its tables"),
             (dict(metrics=ALL["diversity"], cat=d, sqrt_tab=d, n_cats=65, words=1), "cat_words=1 is not ceil"),
             (dict(metrics=ALL["diversity"], cat=d, sqrt_tab=d, n_cats=N.METRICS_MAX_CATS + 1, words=5), "n_cats="),
             (dict(metrics=ALL["ndcg"], disc=None), "ndcg needs the discount table"),
             (dict(metrics=ALL["coverage"]), "coverage needs cover_counts"),
             (dict(metrics=0), "metrics mask"), (dict(metrics=1 << 11), "metrics mask"),
             (dict(ws_bytes=8), "workspace of 8 bytes")]
    for over, text in cases:
        rc = call(**over)
        assert rc == N.DAISY_ERR_ARG, (over, rc)
        assert text in N.last_error(), (over, N.last_error())
        with pytest.raises(ValueError):
            N.check(rc)
    assert N.lib.daisy_ranking_kpis_workspace_bytes(0, 3, 100, 1) == 0
    assert N.lib.daisy_ranking_kpis_workspace_bytes(4, N.METRICS_MAX_CUTOFFS + 1, 100, 1) == 0
    # 1 M lists, five KPIs, six cutoffs, 100 K items with coverage: the partial sums and six bitmaps
    want = (5 * 6 * ((1_000_000 + 255) // 256) * 8 + 255) // 256 * 256 + (6 * ((100_000 + 63) // 64) * 8 + 255) // 256 * 256
    assert N.lib.daisy_ranking_kpis_workspace_bytes(1_000_000, 6, 100_000, 0b101111 | ALL["coverage"]) == want

    # MostPop: topk above the candidate count is refused, as the other models' rank entries refuse it
    rc = N.lib.daisy_pop_rank(d, 100, d, 2, 30, 31, d, d, None)
    assert rc == N.DAISY_ERR_ARG and "topk=31 outside [1, C=30]" in N.last_error()
    rc = N.lib.daisy_pop_rank(d, 100, None, 1, 30, 5, None, d, None)
    assert rc == N.DAISY_ERR_ARG and "item_num and one row when items == NULL" in N.last_error()
    rc = N.lib.daisy_pop_rank(None, 100, d, 2, 30, 5, d, d, None)
    assert rc == N.DAISY_ERR_ARG and "NULL" in N.last_error()
    rc = N.lib.daisy_pop_fit(d, 1, 5, 0, d, d, None)
    assert rc == N.DAISY_ERR_ARG and "item_num=0" in N.last_error()
    rc = N.lib.daisy_pop_fit(d, 1, 5, 10, None, d, None)
    assert rc == N.DAISY_ERR_ARG and "NULL" in N.last_error()
