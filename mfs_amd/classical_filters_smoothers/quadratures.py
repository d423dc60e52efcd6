"""Sigma-point rules, mirroring `SigmaPoints` of `mfs.classical_filters_smoothers.quadratures` (:82-229): the same fields,
factories and methods, in NumPy.

    int z(x) N(x | m, P) dx  ~  sum_i w_i z(chi_i),      chi_i = m + chol(P) xi_i

The Gauss--Hermite rule is built from `numpy.polynomial.hermite_e.hermegauss` (the Golub--Welsch eigenvalue problem of the
probabilists' Hermite polynomials, weights divided by sqrt(2 pi)), not from `np.roots` of a Hermite polynomial as the reference
builds it: the roots of a polynomial given by its coefficients are ill-conditioned at high order, the eigenvalues are not.  The
rule of `order` points per dimension integrates polynomials of degree < 2 order against N(0, I) exactly; d > 1 is the tensor
product, in the reference's point order (the last dimension varies fastest).  The Runge--Kutta helpers of the reference's module
belong to its continuous-discrete filters, which are not here.
"""
import math
from typing import NamedTuple, Optional

import numpy as np
from numpy.polynomial.hermite_e import hermegauss

__all__ = ['SigmaPoints']


class SigmaPoints(NamedTuple):
    """d: dimension; n_points: number of sigma points; w (n_points,): weights; wc: further weights (None for the rules here);
    xi (n_points, d): the points of the standard Normal."""
    d: int
    n_points: int
    w: np.ndarray
    wc: Optional[np.ndarray]
    xi: np.ndarray

    @classmethod
    def cubature(cls, d: int):
        """The spherical cubature rule: 2 d points +- sqrt(d) e_k of weight 1 / (2 d)."""
        d = int(d)
        if d < 1:
            raise ValueError(f'd must be >= 1, got {d}')
        n_points = 2 * d
        xi = math.sqrt(d) * np.concatenate([np.eye(d), -np.eye(d)], axis=0)
        return cls(d=d, n_points=n_points, w=np.full((n_points,), 1. / n_points), wc=None, xi=xi)

    @classmethod
    def unscented(cls, d: int, alpha: float, beta: float, lam: float):
        raise NotImplementedError('Unscented transform is not implemented.')

    @classmethod
    def gauss_hermite(cls, d: int, order: int = 3):
        """The Gauss--Hermite rule with `order` points per dimension: order ** d points."""
        d, order = int(d), int(order)
        if d < 1 or order < 1:
            raise ValueError(f'd and order must be >= 1, got d = {d}, order = {order}')
        x1, w1 = hermegauss(order)
        w1 = w1 / math.sqrt(2. * math.pi)
        grids = np.meshgrid(*([np.arange(order)] * d), indexing='ij')
        table = np.stack([g.reshape(-1) for g in grids], axis=-1)          # (order ** d, d), the last column fastest
        return cls(d=d, n_points=order ** d, w=np.prod(w1[table], axis=-1), wc=None, xi=x1[table])

    def gen_sigma_points(self, m, chol_of_v):
        """chi_i = m + chol_of_v xi_i: (n_points, d)."""
        return np.asarray(m, dtype=np.float64) + np.einsum('ij,...j->...i', np.asarray(chol_of_v, dtype=np.float64), self.xi)

    def expectation(self, evals_of_integrand):
        """sum_i w_i evals[i]: evals (n_points, ...) -> (...)."""
        return np.einsum('i,i...->...', self.w, np.asarray(evals_of_integrand, dtype=np.float64))
