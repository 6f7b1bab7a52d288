"""What the shared surface of the frame-fitted models (EASE, SLiM, ItemKNNCF, UserKNNCF, PureSVD, RP3beta) keeps per class and
no other test states for all of them: the types and shapes of `rank` / `full_rank` / `predict`, their agreement with
`full_rank_users` and with the score matrix, the IndexError texts, the score dtype.  One tiny fitted model per class; every
comparison is an equality."""
import functools

import numpy as np
import pytest
import torch

from conftest import mf_config

pytestmark = pytest.mark.gpu
U, I, TOPK = 6, 5, 3
# 12 (user, item, rating) rows; user 5 has none
ROWS = ((0, 0, 5), (0, 1, 3), (0, 3, 1), (1, 1, 4), (1, 2, 2), (2, 0, 1), (2, 2, 5), (2, 4, 3), (3, 3, 4), (3, 4, 2), (4, 0, 2),
        (4, 1, 5))
KNN = dict(maxk=3, shrink=0, normalize=True, similarity="cosine")
CONFIGS = {"EASE": dict(reg=10), "SLiM": dict(alpha=0.05, elastic=0.1), "ItemKNNCF": KNN, "UserKNNCF": KNN,
           "PureSVD": dict(factors=2), "RP3beta": dict(maxk=3)}
NAMES = list(CONFIGS)


@functools.lru_cache(None)
def fitted(name):
    import pandas as pd
    import daisyrec_amd.model as M
    m = getattr(M, name)(mf_config(user_num=U, item_num=I, topk=TOPK, **CONFIGS[name]))
    u, i, r = zip(*ROWS)
    m.fit(pd.DataFrame({"user": u, "item": i, "rating": r}))
    return m


@functools.lru_cache(None)
def score_matrix(name):
    """[U, I] on the host: float32 from SLiM's _scores, float64 from the others' _rank"""
    m = fitted(name)
    users = torch.arange(U)
    full = m._scores(users) if name == "SLiM" else m._rank(users, None, 0)[0]
    assert full.dtype == (torch.float32 if name == "SLiM" else torch.float64) and tuple(full.shape) == (U, I)
    return full.cpu().numpy()


@functools.lru_cache(None)
def ranked(name):
    """full_rank_users of every user, with the scores"""
    ids, scores = fitted(name).full_rank_users(list(range(U)), return_scores=True)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (U, TOPK) and ids.is_cuda
    return ids.cpu().numpy(), scores


@pytest.mark.parametrize("name", NAMES)
def test_rank_of_an_empty_loader(name):
    out = fitted(name).rank([])
    assert out.dtype == np.int64
    assert out.shape == ((0, TOPK) if name == "PureSVD" else (0,))


@pytest.mark.parametrize("name", NAMES)
def test_rank_of_a_candidate_vector_is_the_full_ranking(name):
    m, want = fitted(name), ranked(name)[0]
    for u in range(U):
        out = m.rank([(torch.tensor([u]), torch.arange(I))])          # one batch, a 1-D candidate vector: all items
        assert out.dtype == np.int64 and out.shape == (1, TOPK)
        assert np.array_equal(out[0], want[u]), (u, out, want[u])


@pytest.mark.parametrize("name", NAMES)
def test_full_rank_is_the_row_of_full_rank_users(name):
    m, want = fitted(name), ranked(name)[0]
    for u in range(U):
        out = m.full_rank(u)
        assert isinstance(out, np.ndarray) and out.dtype == np.int64 and out.shape == (TOPK,)
        assert np.array_equal(out, want[u]), (u, out, want[u])
    assert np.array_equal(score_matrix(name)[5], np.zeros(I))          # the user without a row scores 0 everywhere
    assert m.full_rank(5).tolist() == [0, 1, 2]


@pytest.mark.parametrize("name", NAMES)
def test_predict_is_the_entry_of_the_score_matrix(name):
    m, full = fitted(name), score_matrix(name)
    for u in range(U):
        for i in range(I):
            p = m.predict(u, i)
            assert type(p) is float
            assert np.float64(p).tobytes() == np.float64(full[u, i]).tobytes(), (u, i, p, full[u, i])


@pytest.mark.parametrize("name", NAMES)
def test_ids_out_of_range(name):
    m = fitted(name)
    for call in (lambda: m.predict(U, 0), lambda: m.predict(-1, 0), lambda: m.full_rank(U),
                 lambda: m.rank([(torch.tensor([U]), torch.arange(I))])):
        with pytest.raises(IndexError, match=r"^index out of range: user ids must lie in \[0, 6\)$"):
            call()
    for call in (lambda: m.predict(0, I), lambda: m.predict(0, -1), lambda: m.rank([(torch.tensor([0]), torch.tensor([0, I]))])):
        with pytest.raises(IndexError, match=r"^index out of range: item ids must lie in \[0, 5\)$"):
            call()


@pytest.mark.parametrize("name", NAMES)
def test_score_dtype_of_full_rank_users(name):
    scores = ranked(name)[1]
    assert scores.dtype == (torch.float32 if name == "SLiM" else torch.float64)
    assert tuple(scores.shape) == (U, TOPK)
    # ... and they are the score matrix's entries at the ids
    ids, full = ranked(name)[0], score_matrix(name)
    assert np.array_equal(scores.cpu().numpy(), np.take_along_axis(full, ids, 1))
