"""The MMD misspecification test in numpy float64 -- the model that sf_rbf_rowsum / sf_rbf_subset_sums
(synference_amd/csrc/sf_mmd.hip) and synference_amd/misspecification.py are tested against.

TEST INFRASTRUCTURE ONLY.  The statistic is restated from its definition:

a. ``d2_f32``: the device's squared distance, acc = 0; for c ascending: t = a[c] - b[c]; acc = acc + t * t, every operation
   rounded to float32 on its own (numpy float32 arithmetic does exactly that)
b. ``kernel``: k = exp(-d2 / (2 scale^2)) in float64 on the float32 rows, with the matrix of per-term error bounds
   ``k ((C + 2) 2^-23 |ln k| + ADD)``: the 2 C roundings of d2 and the two of the scaling (the float32 factor c2 and the
   product), then a 1-ulp v_exp_f32 and the conversion (ADD = 2^-22).  The fp64 adds contribute nothing at these sizes.
   The bound of a sum is the sum of its terms' bounds, the bound of an MMD^2 the same linear combination of its sums' bounds.
c. ``mmd2_blocks``: A, B, Cx of two index sets by DIRECT evaluation of the three blocks -- the identity that the device uses
   (``identity_blocks``) is tested against it, not assumed
d. ``null_and_observed``: every shuffle of a case, its p-value and the number of undecidable null values: those within
   (their bound + the observed bound) of the observed statistic.
"""
from __future__ import annotations

import numpy as np

ADD = 2.0 ** -22


def d2_f32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((len(a), len(b)), np.float32)
    for c in range(a.shape[1]):
        t = a[:, c, None] - b[None, :, c]
        acc = acc + t * t
    return acc


def d2_f64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.zeros((len(a), len(b)))
    for c in range(a.shape[1]):
        t = a[:, c, None] - b[None, :, c]
        out += t * t
    return out


def kernel(a, b, scale):
    """-> K [len(a), len(b)] float64 and the matrix of per-term bounds."""
    C = np.asarray(a).shape[1]
    la = -d2_f64(a, b) / (2.0 * float(scale) ** 2)
    K = np.exp(la)
    return K, K * ((C + 2) * 2.0 ** -23 * np.abs(la) + ADD)


def offdiag_sum(K):
    return float(K.sum() - np.trace(K))


def scale_model(z, pick):
    """numpy.median of the Euclidean distances over all pairs i < j of the rows ``pick`` of z."""
    a = np.asarray(z, np.float64)[pick]
    d = np.sqrt(d2_f64(a, a))
    return float(np.median(d[np.triu_indices(len(a), 1)]))


def mmd2(A, B, Cx, m, n):
    return A / (m * (m - 1)) + B / (n * (n - 1)) - 2.0 * Cx / (m * n)


def mmd2_bound(Ab, Bb, Cb, m, n):
    return Ab / (m * (m - 1)) + Bb / (n * (n - 1)) + 2.0 * Cb / (m * n)


def mmd2_blocks(K, S, T):
    """A, B, Cx of the sets S and T of one kernel matrix, each block summed directly."""
    KS, KT = K[np.ix_(S, S)], K[np.ix_(T, T)]
    return offdiag_sum(KS), offdiag_sum(KT), float(K[np.ix_(S, T)].sum())


def identity_blocks(K, S):
    """The same three sums from the row sums r_i = sum_{j != i} K_ij and the S x S block alone."""
    r = K.sum(1) - np.diag(K)
    R = float(r.sum())
    A = offdiag_sum(K[np.ix_(S, S)])
    Cx = float(r[S].sum()) - A
    return A, R - A - 2.0 * Cx, Cx


def null_and_observed(z, z_obs, subsets, scale):
    """Everything the device computes for one case, in float64 with its bounds (module docstring)."""
    z, z_obs = np.asarray(z, np.float32), np.asarray(z_obs, np.float32)
    N, M = len(z), len(z_obs)
    K, E = kernel(z, z, scale)
    Ko, Eo = kernel(z_obs, z_obs, scale)
    Kx, Ex = kernel(z_obs, z, scale)
    r, r_b = K.sum(1) - np.diag(K), E.sum(1) - np.diag(E)
    R, R_b = float(r.sum()), float(r_b.sum())
    row_o, row_o_b = Ko.sum(1) - np.diag(Ko), Eo.sum(1) - np.diag(Eo)
    row_x, row_x_b = Kx.sum(1), Ex.sum(1)
    A_o, Cx_o = float(row_o.sum()), float(row_x.sum())
    obs = mmd2(A_o, R, Cx_o, M, N)
    obs_b = mmd2_bound(float(row_o_b.sum()), R_b, float(row_x_b.sum()), M, N)
    out = dict(r=r, r_b=r_b, R=R, R_b=R_b, row_o=row_o, row_o_b=row_o_b, row_x=row_x, row_x_b=row_x_b, A_o=A_o, Cx_o=Cx_o,
               mmd2=obs, mmd2_b=obs_b)
    n = N - M
    pair, pair_b, picked, picked_b, null, null_b = ([] for _ in range(6))
    everything = np.arange(N)
    for S in np.asarray(subsets, np.int64):
        T = np.setdiff1d(everything, S)
        A, B, Cx = mmd2_blocks(K, S, T)
        Ab, Bb, Cb = mmd2_blocks(E, S, T)
        pair.append(A), pair_b.append(Ab), picked.append(float(r[S].sum())), picked_b.append(float(r_b[S].sum()))
        null.append(mmd2(A, B, Cx, M, n)), null_b.append(mmd2_bound(Ab, Bb, Cb, M, n))
    null, null_b = np.array(null), np.array(null_b)
    out.update(pair=np.array(pair), pair_b=np.array(pair_b), picked=np.array(picked), picked_b=np.array(picked_b), null=null,
               null_b=null_b, p_value=float(np.mean(null > obs)),
               undecidable=int((np.abs(null - obs) <= null_b + obs_b).sum()),
               smallest_gap=float(np.abs(null - obs).min()), largest_bound=float((null_b + obs_b).max()))
    return out
