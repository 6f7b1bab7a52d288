"""Plain numpy / scipy fp64 restatement of EASE as daisyrec_amd computes it (test infrastructure): the Gram
matrix of the fp32 ratings plus reg on the diagonal, its Cholesky factor, the triangular inverse, P = T^T T and
B = -P / diag(P) with a zero diagonal.  The reference takes the same P from np.linalg.inv (LU)."""
import numpy as np
import scipy.linalg

#           tag: (U, I, reg, density, seed)
FIXTURES = {"tiny": (40, 23, 200.0, .20, 0),            # less than one block
            "ragged": (120, 97, 200.0, .10, 1),         # one block plus a tail that is not a multiple of 16
            "oneplus": (30, 65, 10.0, .20, 2),          # a block plus one column
            "blocks": (300, 257, 200.0, .08, 3),        # four blocks plus one column
            "wide": (64, 130, 0.5, .10, 4),             # U < I: X^T X is singular, only reg keeps the system definite
            "dup": (50, 40, 200.0, .20, 5)}             # duplicate pairs, one user without history, one unrated item
DUP_EMPTY_USER, DUP_UNRATED_ITEM = 7, 11


def triples(tag):
    """(user, item, rating) of a fixture: popularity-skewed items, integer ratings 1..5 (so that G is exact in fp32).
    Every user has a history, except DUP_EMPTY_USER of 'dup'; 'dup' also repeats 30 of its pairs and leaves
    DUP_UNRATED_ITEM without a rating."""
    U, I, _, dens, seed = FIXTURES[tag]
    rng = np.random.RandomState(seed)
    pop = rng.zipf(1.3, I).clip(1, 50).astype(float)
    pop /= pop.max()
    M = rng.rand(U, I) < (dens * (0.3 + pop))[None, :] * 2
    for u in np.nonzero(~M.any(1))[0]:
        M[u, rng.randint(I)] = True
    if tag == "dup":
        M[DUP_EMPTY_USER, :] = False
        M[:, DUP_UNRATED_ITEM] = False
        for u in np.nonzero(~M.any(1))[0]:
            if u != DUP_EMPTY_USER:
                M[u, 0] = True
    u, i = np.nonzero(M)
    r = rng.randint(1, 6, len(u)).astype(float)
    if tag == "dup":
        again = rng.permutation(len(u))[:30]
        u, i, r = np.concatenate([u, u[again]]), np.concatenate([i, i[again]]), np.concatenate([r, rng.randint(1, 6, 30)])
        order = rng.permutation(len(u))
        u, i, r = u[order], i[order], r[order].astype(float)
    return u, i, r


def dense(u, i, r, U, I):
    """X [U, I] float64 with duplicate (user, item) pairs summed, rounded through fp32 like the reference's astype."""
    X = np.zeros((U, I))
    np.add.at(X, (np.asarray(u), np.asarray(i)), np.asarray(r, dtype=np.float64))
    return X.astype(np.float32).astype(np.float64)


def system(X, reg):
    """A = fp32(X^T X) + reg I in fp64 (EASERecommender.py:37-39)"""
    G = (X.astype(np.float32).T @ X.astype(np.float32)).astype(np.float64)
    return G + reg * np.eye(X.shape[1])


def spd_inverse(A):
    """P = A^-1 by the Cholesky route: A = L L^T, T = L^-1, P = T^T T"""
    L = np.linalg.cholesky(A)
    T = scipy.linalg.solve_triangular(L, np.eye(A.shape[0]), lower=True)
    return T.T @ T


def weights(P):
    """B = -P / diag(P) (column j divided by P[j, j]) with a zero diagonal (EASERecommender.py:42-43)"""
    B = -P / np.diag(P)
    np.fill_diagonal(B, 0.0)
    return B


def fit(X, reg):
    """-> B float64 [I, I]"""
    return weights(spd_inverse(system(np.asarray(X, dtype=np.float64), reg)))


# ---- scores and lists -----------------------------------------------------------------------------------------------------
def scores(X, B, users, cands):
    """[len(users), C] at the candidates cands [len(users), C]"""
    full = X[users] @ B
    return np.take_along_axis(full, cands, axis=1)


def rank_lists(sc, cands, topk):
    """ids of the topk largest scores per row, ties by position (stable)"""
    order = np.argsort(-sc, axis=1, kind="stable")[:, :topk]
    return np.take_along_axis(cands, order, axis=1)


def min_top_gap(sc, top=11):
    """the smallest gap between adjacent scores among every row's `top` best"""
    s = -np.sort(-sc, axis=1)[:, :top]
    return float(np.min(s[:, :-1] - s[:, 1:])) if s.shape[1] > 1 else np.inf
