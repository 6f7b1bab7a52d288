"""The models fitted from a DataFrame, on the host: what `fit` says about a bad frame (message by message, with the class's
name in it), that a bad frame is refused BEFORE the missing device is, what the ranking entry points say before `fit`, and
the class relations and package exports that outside code relies on.  Nothing here needs a device."""
import inspect
import re

import numpy as np
import pytest
import torch

from conftest import mf_config

U, I = 3, 4
CONFIGS = {
    "EASE": dict(reg=10.0),
    "SLiM": dict(alpha=0.05, elastic=0.1),
    "PureSVD": dict(factors=2),
    "ItemKNNCF": dict(maxk=3, shrink=0.0, normalize=True, similarity="cosine"),
    "UserKNNCF": dict(maxk=3, shrink=0.0, normalize=True, similarity="cosine"),
    "RP3beta": dict(maxk=3),
    "P3alpha": dict(maxk=3),
    "IALS": dict(factors=2, reg=0.1, alpha=1.0, epochs=1),
    "MostPop": dict(),
}
NAMES = list(CONFIGS)
HAS_POSITIONS = ("SLiM", "PureSVD", "ItemKNNCF", "UserKNNCF", "RP3beta", "P3alpha", "IALS")
NO_DEVICE = "no HIP device visible"


def make(name, **over):
    import daisyrec_amd.model as M
    return getattr(M, name)(mf_config(user_num=U, item_num=I, topk=3, **{**CONFIGS[name], **over}))


def frame(u, i, r):
    import pandas as pd
    return pd.DataFrame({"user": u, "item": i, "rating": r})


def refused(model, df, message):
    with pytest.raises(ValueError, match="^" + re.escape(message)):
        model.fit(df)


@pytest.mark.parametrize("name", NAMES)
def test_bad_ids_are_named_with_the_class(name):
    m = make(name)
    if name != "MostPop":                                 # (MostPop reads the item column only)
        refused(m, frame([0, 3], [0, 1], [1., 1.]), f"{name}.fit: user id 3 outside [0, 3)")
        refused(m, frame([0, -1], [0, 1], [1., 1.]), f"{name}.fit: user id -1 outside [0, 3)")
        refused(m, frame([0, 1.5], [0, 1], [1., 1.]), f"{name}.fit: column 'user' holds non-integer ids")
    refused(m, frame([0, 1], [0, 4], [1., 1.]), f"{name}.fit: item id 4 outside [0, 4)")
    refused(m, frame([0, 1], [-2, 1], [1., 1.]), f"{name}.fit: item id -2 outside [0, 4)")
    refused(m, frame([0, 1], [0, 2.5], [1., 1.]), f"{name}.fit: column 'item' holds non-integer ids")


@pytest.mark.parametrize("name", [n for n in NAMES if n != "MostPop"])
def test_bad_ratings_are_named_with_the_class(name):
    m = make(name)
    refused(m, frame([0, 1], [0, 1], [1., np.inf]), f"{name}.fit: column 'rating' holds a value that is not finite")
    refused(m, frame([0, 1], [0, 1], [np.nan, 1.]), f"{name}.fit: column 'rating' holds a value that is not finite")
    # the user column is checked first, then the item column, then the ratings
    refused(m, frame([0, 3], [0, 4], [1., np.inf]), f"{name}.fit: user id 3 outside [0, 3)")
    refused(m, frame([0, 1], [0, 4], [1., np.inf]), f"{name}.fit: item id 4 outside [0, 4)")


def test_the_two_checks_of_single_families():
    refused(make("IALS"), frame([0, 1], [0, 1], [1., -1.]), "IALS.fit: column 'rating' holds a negative value (-1.0): a confidence")
    refused(make("IALS"), frame([0, 1], [0, 1], [1., np.inf]), "IALS.fit: column 'rating' holds a value that is not finite")
    for name in ("RP3beta", "P3alpha"):
        refused(make(name, implicit=False), frame([0, 1], [0, 1], [1., 0.]),
                f"{name}.fit: column 'rating' holds 0.0: a transition probability needs ratings > 0")
        refused(make(name, implicit=False), frame([0, 1], [0, 1], [1., np.inf]),
                f"{name}.fit: column 'rating' holds a value that is not finite")
    if not torch.cuda.is_available():                     # implicit=True takes a zero rating: the device is missed next
        with pytest.raises(RuntimeError, match=NO_DEVICE):
            make("RP3beta").fit(frame([0, 1], [0, 1], [1., 0.]))


@pytest.mark.parametrize("name", NAMES)
def test_a_missing_column_is_a_key_error(name):
    m = make(name)
    with pytest.raises(KeyError):
        m.fit(frame([0], [0], [1.]).rename(columns={"item": "label"}))
    if name != "MostPop":
        with pytest.raises(KeyError):
            m.fit(frame([0], [0], [1.]).rename(columns={"rating": "label"}))
        with pytest.raises(KeyError):
            m.fit(frame([0], [0], [1.]).rename(columns={"user": "label"}))


def test_the_configured_column_names():
    """EASE, IALS and MostPop read the columns the config names, the others the literals 'user' / 'item' / 'rating'."""
    renamed = frame([0, 3], [0, 4], [1., np.inf]).rename(columns={"user": "uid", "item": "iid", "rating": "r"})
    names = dict(UID_NAME="uid", IID_NAME="iid", INTER_NAME="r")
    for name in ("EASE", "IALS"):
        refused(make(name, **names), renamed, f"{name}.fit: user id 3 outside [0, 3)")
        renamed_ok = renamed.assign(uid=[0, 1], iid=[0, 1])
        refused(make(name, **names), renamed_ok, f"{name}.fit: column 'r' holds a value that is not finite")
        refused(make(name, **names), renamed_ok.assign(uid=[0, 1.5]), f"{name}.fit: column 'uid' holds non-integer ids")
    refused(make("MostPop", **names), renamed, "MostPop.fit: iid id 4 outside [0, 4)")
    refused(make("MostPop", **names), renamed.assign(iid=[0, 0.5]), "MostPop.fit: column 'iid' holds non-integer ids")
    for name in ("SLiM", "PureSVD", "ItemKNNCF", "UserKNNCF", "RP3beta", "P3alpha"):
        with pytest.raises(KeyError):
            make(name, **names).fit(renamed)
        refused(make(name, **names), frame([0, 3], [0, 1], [1., 1.]), f"{name}.fit: user id 3 outside [0, 3)")


@pytest.mark.parametrize("name", NAMES)
def test_the_device_is_missed_after_the_frame(name):
    if torch.cuda.is_available():
        return                                            # (with a device these frames fit: tests/test_gpu_*.py)
    m = make(name)
    for df in (frame([0, 1], [0, 1], [1., 1.]),
               frame([0., 1.], [0., 1.], [1., 1.])):      # whole numbers in a float column are ids
        with pytest.raises(RuntimeError, match=NO_DEVICE):
            m.fit(df)
    refused(m, frame([0, 1], [0, 4], [1., 1.]), f"{name}.fit: item id 4 outside [0, 4)")      # ... never instead of them


@pytest.mark.parametrize("name", NAMES)
def test_before_fit(name):
    m = make(name)
    unfitted = f"^{name}: " + re.escape("fit(train_set) has not been called") if torch.cuda.is_available() else NO_DEVICE
    with pytest.raises(RuntimeError, match=unfitted):
        m.full_rank(0)
    if name == "MostPop":                                 # it has neither: AbstractRecommender answers
        with pytest.raises(NotImplementedError, match="MostPop has no full_rank_users"):
            m.full_rank_users([0])
    else:
        with pytest.raises(RuntimeError, match=unfitted):
            m.full_rank_users([0])
    if name in HAS_POSITIONS:
        with pytest.raises(RuntimeError, match=unfitted):
            m.full_rank_positions([0], {0: {1}})
    else:
        with pytest.raises(NotImplementedError, match=f"{name} has no full_rank_positions.*EASE and NeuMF follow"):
            m.full_rank_positions([0], {0: {1}})


def test_class_relations_and_exports():
    import daisyrec_amd.model as M
    from daisyrec_amd.model.KNNCFRecommender import _KNNCF
    for name in NAMES:
        assert issubclass(getattr(M, name), M.GeneralRecommender), name
    for name in ("ItemKNNCF", "UserKNNCF", "RP3beta", "P3alpha"):
        assert issubclass(getattr(M, name), _KNNCF), name
    assert issubclass(M.P3alpha, M.RP3beta)
    assert not issubclass(M.RP3beta, M.ItemKNNCF)
    assert not hasattr(M, "__all__")
    exported = sorted(n for n, v in vars(M).items() if inspect.isclass(v))
    assert exported == sorted([
        "AbstractRecommender", "AERecommender", "GeneralRecommender", "MF", "FM", "NeuMF", "LightGCN", "NGCF", "NFM",
        "Item2Vec", "VAECF", "SLiM", "PureSVD", "EASE", "IALS", "ItemKNNCF", "UserKNNCF", "P3alpha", "RP3beta", "MostPop"])
    for name in NAMES:                                    # the private state tests and tools read
        m = make(name)
        for attr in {"EASE": ("_csr", "_B"), "SLiM": ("_csr", "_W", "_scores", "_check_users"),
                     "PureSVD": ("_user_vec", "_item_vec", "_rank"), "IALS": (), "MostPop": ()}.get(
                         name, ("_csr", "_csr_t", "_W", "_L", "_R", "_rank")):
            assert hasattr(m, attr), (name, attr)
        assert callable(m._fitted)
