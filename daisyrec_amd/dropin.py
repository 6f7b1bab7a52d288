"""Make an unmodified daisyRec driver (run_examples/test.py, tune.py) train MF through
the HIP path: rebinds the names those scripts import (test.py:4,21-22; tune.py:7).

    import daisyrec_amd.dropin as d; d.install()          # before `import run_examples.test`

or, where the reference checkout exists:
    python tools/run_daisy_example.py --daisy /path/to/daisyRec -- --algo_name mf ...
"""
from __future__ import annotations

import importlib


# what install(metrics=True) rebinds in daisy.utils.metrics
METRICS_NAMES = ("metrics_name_config", "calc_ranking_results", "Metric", "Coverage", "Popularity", "Diversity", "Precision",
                 "Recall", "MRR", "MAP", "NDCG", "HR", "AUC", "F1")


# what install(prep=True) rebinds in daisy.utils.splitter (and Preprocessor in daisy.utils.loader)
SPLITTER_NAMES = ("TestSplitter", "ValidationSplitter", "split_test", "split_validation")


# what install(history=True) rebinds in daisy.utils.utils (and AEDataset in daisy.utils.dataset)
HISTORY_NAMES = ("get_history_matrix", "get_inter_matrix")


def install(sampler=False, front_end=False, metrics=False, prep=False, history=False):
    """Patch `daisy.model.MFRecommender.MF` (and the other mirrored recommenders) in place.
    history: also `daisy.utils.utils.get_history_matrix` / `get_inter_matrix` and `daisy.utils.dataset.AEDataset` (the padded
    histories of multi-vae, the interaction matrix of lightgcn / ngcf and the AE loader's users from the device instead of
    Python loops over the rows).  Like front_end: call before the driver module is imported
    (test.py:22-23 binds the names at import).  Without it both modules' names are left untouched.
    prep: also `daisy.utils.loader.Preprocessor` and `daisy.utils.splitter`'s `TestSplitter`, `ValidationSplitter`,
    `split_test`, `split_validation` (dedup, k-core, encoding, time sort and every split on the device instead of Python
    loops over rows and users; DESIGN.md section 21 lists the deviations).  Like front_end: call before the driver module
    is imported (test.py:5-6 binds the classes at import).  Without it both modules are left untouched.
    metrics: also `daisy.utils.metrics` - `calc_ranking_results`, `Metric`, `metrics_name_config` and the eleven KPI
    functions (one device pass for all cutoffs instead of a Python loop per user, KPI and cutoff).  Like front_end: call
    before the driver module is imported (test.py:18 binds `calc_ranking_results`, tune.py:23 the KPI functions at import).
    sampler: also the negative sampler (device generator: same distribution, different stream than MT19937).
    front_end: also `daisy.utils.utils.get_ur / get_ir` (same dicts, built from one sort instead of a Python row
    loop) and `build_candidates_set` (device generator) - what makes the drivers usable beyond ml-100k sizes
    (SURVEY.md section 8f rank 1).  Call before the driver module is imported (it binds these names at import)."""
    from .model.MFRecommender import MF
    from .model.FMRecommender import FM

    ref_mf = importlib.import_module("daisy.model.MFRecommender")
    ref_mf.MF = MF
    ref_fm = importlib.import_module("daisy.model.FMRecommender")
    ref_fm.FM = FM
    from .model.NeuMFRecommender import NeuMF
    ref_nm = importlib.import_module("daisy.model.NeuMFRecommender")
    ref_nm.NeuMF = NeuMF
    from .model.Item2VecRecommender import Item2Vec
    ref_iv = importlib.import_module("daisy.model.Item2VecRecommender")
    ref_iv.Item2Vec = Item2Vec
    from .model.LightGCNRecommender import LightGCN
    try:                                   # imports scipy; the reference module itself needs it too
        ref_lg = importlib.import_module("daisy.model.LightGCNRecommender")
        ref_lg.LightGCN = LightGCN
    except ImportError:
        pass
    from .model.NGCFRecommender import NGCF
    try:                                   # the reference module imports scipy as well
        ref_ng = importlib.import_module("daisy.model.NGCFRecommender")
        ref_ng.NGCF = NGCF
    except ImportError:
        pass
    from .model.NFMRecommender import NFM
    ref_nf = importlib.import_module("daisy.model.NFMRecommender")
    ref_nf.NFM = NFM
    from .model.VAECFRecommender import VAECF
    ref_vae = importlib.import_module("daisy.model.VAECFRecommender")
    ref_vae.VAECF = VAECF
    from .model.SLiMRecommender import SLiM
    try:                                   # the reference module imports scipy and scikit-learn
        ref_slim = importlib.import_module("daisy.model.SLiMRecommender")
        ref_slim.SLiM = SLiM
    except ImportError:
        pass
    from .model.PureSVDRecommender import PureSVD
    try:                                   # the reference module imports scipy and scikit-learn
        ref_psvd = importlib.import_module("daisy.model.PureSVDRecommender")
        ref_psvd.PureSVD = PureSVD
    except ImportError:
        pass
    from .model.EASERecommender import EASE
    try:                                   # the reference module imports scipy
        ref_ease = importlib.import_module("daisy.model.EASERecommender")
        ref_ease.EASE = EASE
    except ImportError:
        pass
    from .model.KNNCFRecommender import ItemKNNCF, UserKNNCF
    try:                                   # the reference module imports scipy
        ref_knn = importlib.import_module("daisy.model.KNNCFRecommender")
        ref_knn.ItemKNNCF, ref_knn.UserKNNCF = ItemKNNCF, UserKNNCF
    except ImportError:
        pass
    from .model.PopRecommender import MostPop
    ref_pop = importlib.import_module("daisy.model.PopRecommender")
    ref_pop.MostPop = MostPop
    if metrics:
        from .utils import metrics as M

        ref_m = importlib.import_module("daisy.utils.metrics")
        for name in METRICS_NAMES:
            setattr(ref_m, name, getattr(M, name))
    if prep:
        from .utils import loader as L, splitter as S

        ref_l = importlib.import_module("daisy.utils.loader")
        ref_l.Preprocessor = L.Preprocessor
        ref_sp = importlib.import_module("daisy.utils.splitter")
        for name in SPLITTER_NAMES:
            setattr(ref_sp, name, getattr(S, name))
    if sampler:
        from .utils.sampler import BasicNegtiveSampler

        from .utils.sampler import SkipGramNegativeSampler

        ref_s = importlib.import_module("daisy.utils.sampler")
        ref_s.BasicNegtiveSampler = BasicNegtiveSampler
        ref_s.SkipGramNegativeSampler = SkipGramNegativeSampler
    if front_end:
        from .utils import utils as U

        ref_u = importlib.import_module("daisy.utils.utils")
        ref_u.get_ur, ref_u.get_ir = U.get_ur, U.get_ir
        ref_u.build_candidates_set = U.build_candidates_set
    if history:
        from .utils import dataset as D, utils as U

        ref_u = importlib.import_module("daisy.utils.utils")
        for name in HISTORY_NAMES:
            setattr(ref_u, name, getattr(U, name))
        ref_d = importlib.import_module("daisy.utils.dataset")
        ref_d.AEDataset = D.AEDataset
    return MF
