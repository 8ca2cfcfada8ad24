"""Multilinear polynomials over Fr on the GPU, from bn_amd.fr_mle_eq, bn_amd.fr_mle_fold, bn_amd.fr_mle_quotients and the sparse linear map
(bn_amd.fr_dot_batch).

A multilinear polynomial of nv variables is the table of its 2^nv values over the hypercube, value first at index 0: the entry at index i is
the value at the point whose variable j is bit j of i (Fr values, or an (n,4) uint64 array of Montgomery limbs).  A point is a list of nv
Fr, variable 0 first.  fold binds the MOST significant variable, so nv folds by point[nv-1], point[nv-2], .. point[0] leave the value at
the point - the order in which bn_amd.sumcheck binds its challenges."""
import numpy as np

from .api import Fr, _scalar_array, default_engine
from .engine import _mle_eq_args, _mle_fold_args, _mle_quotients_args


def eq_table(point, limbs=False, engine=None):
    """[eq(point, x) for x in the hypercube], a list of 2^len(point) Fr - or, limbs=True, the (2^nv, 4) uint64 array: eq(z, x) = prod_j
    (z_j x_j + (1 - z_j)(1 - x_j)) is one where x == z on the hypercube and zero elsewhere on it.  ONE call; no variables give [one]."""
    z = _mle_eq_args(_scalar_array(point))
    out = (engine or default_engine()).fr_mle_eq(z)
    return out if limbs else [Fr.from_limbs(r) for r in out]


def fold(table, r, limbs=False, engine=None):
    """the table with its most significant variable bound to r: [t[i] + r * (t[i + n/2] - t[i]) for i < n/2], a list of Fr - or, limbs=True, the
    array.  An (n, k, 4) array holds k tables index-major and all are folded in the one call.  ValueError for an odd length."""
    if isinstance(table, np.ndarray) and table.ndim == 3:
        A, rr = _mle_fold_args(table, r)
    else:
        A, rr = _mle_fold_args(_scalar_array(table), r)
    out = (engine or default_engine()).fr_mle_fold(A, rr)
    return out if limbs or out.ndim != 2 else [Fr.from_limbs(x) for x in out]


def evaluate(table, point, engine=None):
    """the multilinear polynomial with these values at `point`, an Fr: sum_i table[i] * eq(point, i) - ONE eq table and ONE inner product
    (fr_dot_batch without an index), not len(point) folds.  ValueError unless len(table) == 2^len(point)."""
    T, z = _scalar_array(table), _mle_eq_args(_scalar_array(point))
    if T.shape[0] != 1 << z.shape[0]:
        raise ValueError(f"table holds {T.shape[0]} values but point has {z.shape[0]} variables: 2^{z.shape[0]} are needed")
    e = engine or default_engine()
    return Fr.from_limbs(e.fr_dot_batch(T, e.fr_mle_eq(z), [0, T.shape[0]])[0])


def quotients(table, point, limbs=False, engine=None):
    """(value, [q_0, .., q_{nv-1}]): the value at `point`, an Fr, and the quotient tables of the opening there - q_j a list of 2^j Fr with
    f(x) - f(point) = sum_j (x_j - point_j) q_j(x_0 .. x_{j-1}).  ONE call (fr_mle_quotients); limbs=True gives the (2^j, 4) uint64 arrays, views
    of its one output.  ValueError unless len(table) == 2^len(point)."""
    T, z = _mle_quotients_args(_scalar_array(table), _scalar_array(point))
    out = (engine or default_engine()).fr_mle_quotients(T, z)
    qs = [out[1 << j:2 << j] for j in range(z.shape[0])]
    return Fr.from_limbs(out[0]), qs if limbs else [[Fr.from_limbs(r) for r in q] for q in qs]
