"""Support for the N-D filter tests (d = 2 and d = 3), everything that does not depend on the dimension, each defined once:
the graded-lex tables, the moments of a Normal start, the moment error with its natural-magnitude floor, one runner for the
device filters and one for oracle/multi_dims.py, the comparison of a device run with an oracle run, the bit comparison of two
device runs and the likelihoods built from a factor spec.  The models live in tests/nd_envelope_models.py (d = 2) and
tests/nd3_models.py (d = 3).  A plain module: no fixtures, nothing runs on import; tests/test_host_nd_support.py checks what
the assertions here accept and refuse, tests/test_host_test_layers.py that no support module imports a test module."""
import functools
import math

import numpy as np

from mfs_amd import stats, sym
from mfs_amd.multi_dims import filtering
from mfs_amd.multi_dims.multi_indices import generate_graded_lexico_multi_indices, gram_and_hankel_indices_graded_lexico
from oracle import models as om, multi_dims as omd, one_dim as o1
from tests.plan_api import assert_same_bits

RTOL = 1e-6
MODES = ('raw', 'central', 'scaled')
MOMENTS_OF = {'raw': 'rms', 'central': 'cms', 'scaled': 'scms'}       # mode -> its key in a start built by `initial`


# ---- tables and starts --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables(d, N):
    """(multi-indices up to degree 2N - 1, Gram and Hankel index tables) in graded-lex order; shared, not to be written to."""
    return generate_graded_lexico_multi_indices(d, 2 * N - 1), gram_and_hankel_indices_graded_lexico(N, d)


def initial(mi, mean, cov):
    """Raw, central and scaled moments of N(mean, cov) on the table, with the mean and the scales; d is that of the table."""
    mean, cov = np.asarray(mean, dtype=float), np.asarray(cov, dtype=float)
    rms = np.array([omd.raw_moments_mvn_kan(mean, cov, n) for n in mi])
    cms = np.array([omd.raw_moments_mvn_kan(np.zeros(mi.shape[1]), cov, n) for n in mi])
    scale = np.sqrt(np.diag(cov))
    return {'rms': rms, 'cms': cms, 'scms': cms / np.prod(scale ** mi, axis=-1), 'mean': mean, 'scale': scale}


def stack_initial(states):
    return {k: np.stack([s[k] for s in states]) for k in states[0]}


def host_drift(m):
    """The drift of a model (a callable on a sequence of the state variables) in the form the host traces: an object array."""
    return lambda x: np.array(m.drift(x), dtype=object)


def host_disp(m):
    return lambda x: np.array(m.disp(x), dtype=object)


# ---- errors and assertions ----------------------------------------------------------------------------------------------
def second(mi):
    """Where the table holds the second moment of each component (the multi-indices 2 e_k)."""
    mi = np.asarray(mi)
    d = mi.shape[1]
    return [int(np.where((mi == 2 * np.eye(d, dtype=int)[k]).all(axis=1))[0][0]) for k in range(d)]


def moment_err(got, ref, mi):
    """(T, z) relative error per moment with the natural magnitude prod_k sigma_k^{n_k} as the floor of the denominator:
    first-order central moments and odd moments of near-symmetric laws are rounding noise around zero."""
    got, ref, mi = np.asarray(got), np.asarray(ref), np.asarray(mi)
    m2 = np.abs(ref[:, second(mi)])                                                # (T, d): E[(x_k - c_k)^2] or E[x_k^2]
    natural = np.prod(np.sqrt(m2)[:, None, :] ** mi[None, :, :], axis=-1)          # (T, z)
    scale = np.maximum(np.abs(ref), natural * 1e-2 + 1e-300)
    return np.abs(got - ref) / scale


def assert_moments(got, ref, mi, rtol):
    """moment_err <= rtol wherever the reference is finite, and the same NaN pattern."""
    assert np.array_equal(np.isnan(np.asarray(got)), np.isnan(np.asarray(ref)))
    err = moment_err(got, ref, mi)
    assert np.nanmax(err) <= rtol, f'max scaled error {np.nanmax(err):.3e} > {rtol}'


def first_bad(r):
    """The first step at which a single-replicate run has a non-finite moment, mean or scale; -1 if none."""
    bad = ~np.isfinite(r['m']).all(axis=1)
    for k in ('mean', 'scale'):
        if k in r:
            bad |= ~np.isfinite(r[k]).all(axis=1)
    return int(np.argmax(bad)) if bad.any() else -1


def all_finite(r):
    return bool(np.isfinite(r['nell']) and all(np.all(np.isfinite(r[k])) for k in ('m', 'mean', 'scale') if k in r))


def same_bits(a, b, keys=('m', 'mean', 'scale', 'nell', 'fn')):
    """Two result dicts of `run_device` hold the same bits, and the same keys of `keys`."""
    assert_same_bits([a.get(k) for k in keys], [b.get(k) for k in keys], names=keys)


# ---- the runners --------------------------------------------------------------------------------------------------------
def run_device(mode, fns, sig, pdf, ys, mi, inds, st, stable=False):
    """The device filter of one mode on batched measurements -> dict(m, mean, scale, nell, fn)."""
    mp = (mi, inds)
    if mode == 'raw':
        m, nell, fn = filtering.moment_filter_nd_rms((fns[0], sig), pdf, ys, mp, st['rms'], stable, return_first_nan=True)
        return {'m': m, 'nell': nell, 'fn': fn}
    if mode == 'central':
        m, mean, nell, fn = filtering.moment_filter_nd_cms((fns[1], sig), fns[3], pdf, ys, mp, st['cms'], st['mean'], stable,
                                                           return_first_nan=True)
        return {'m': m, 'mean': mean, 'nell': nell, 'fn': fn}
    m, mean, scale, nell, fn = filtering.moment_filter_nd_scms((fns[2], sig), fns[4], pdf, ys, mp, st['scms'], st['mean'],
                                                               st['scale'], stable, return_first_nan=True)
    return {'m': m, 'mean': mean, 'scale': scale, 'nell': nell, 'fn': fn}


def run_oracle(mode, ofns, sig, opdf, ys, mi, inds, st, stable=False, completed=False):
    """oracle/multi_dims.py on one replicate (T, ny) -> dict(m, mean, scale, nell); raw mode reports its means as the
    first-order raw moments.  With `completed` the dict also says at which step one of the two rules first took the LDL^T
    completion (a pivot not > 0, stable=True only), -1 if none: oracle.one_dim.ldl is watched for the length of the run."""
    mp = (mi, inds)
    calls, first = [0], [-1]
    ldl0 = o1.ldl

    def spy(mat):
        l, d = ldl0(mat)
        if first[0] < 0 and not np.all(d > 0):
            first[0] = calls[0]
        calls[0] += 1
        return l, d
    if completed:
        o1.ldl = spy
    try:
        if mode == 'raw':
            m, nell = omd.moment_filter_nd_rms((ofns[0], sig), opdf, ys, mp, st['rms'], stable)
            out = {'m': m, 'nell': nell}
        elif mode == 'central':
            m, mean, nell = omd.moment_filter_nd_cms((ofns[1], sig), ofns[3], opdf, ys, mp, st['cms'], st['mean'], stable)
            out = {'m': m, 'mean': mean, 'nell': nell}
        else:
            m, mean, scale, nell = omd.moment_filter_nd_scms((ofns[2], sig), ofns[4], opdf, ys, mp, st['scms'], st['mean'],
                                                             st['scale'], stable)
            out = {'m': m, 'mean': mean, 'scale': scale, 'nell': nell}
    finally:
        o1.ldl = ldl0
    if completed:
        out['completed'] = first[0] // 2 if first[0] >= 0 else -1
    return out


# ---- a device run against an oracle run ---------------------------------------------------------------------------------
def assert_state(got, b, ref, mi, upto, rtol, tag=''):
    """Moments, means and scales of replicate b of `got` against `ref` on steps < upto: relative, with the natural
    magnitude as the floor (1e-2 sd for a mean)."""
    if upto <= 0:
        return
    assert_moments(got['m'][b, :upto], ref['m'][:upto], mi, rtol)
    sd = ref['scale'][:upto] if 'scale' in ref else np.sqrt(np.abs(ref['m'][:upto][:, second(mi)]))
    for k in ('mean', 'scale'):
        if k in ref:
            err = np.abs(got[k][b, :upto] - ref[k][:upto]) / np.maximum(np.abs(ref[k][:upto]), 1e-2 * sd)
            assert err.max() <= rtol, f'{tag}: {k} error {err.max():.3e} > {rtol}'


def compare(got, b, ref, mi, inds, tag=''):
    """Replicate b of a device run against the oracle's run of it: 1e-6 on every step before either side poisons, and the
    NaN criterion of tests/test_gpu_fuzz_1d.py -- a poisoning the other side does not share (or shares at another step)
    is accepted only where the later side's Gram matrix around that step is numerically singular (cond >= 1e13).  With
    stable=True, the comparison ends at the first step whose rule takes the LDL^T completion: its K_k have norms
    ~ 1 / eps^2 and both eigensolvers are accurate relative to those norms only (the criterion of
    tests/test_gpu_nd3.py::test_stable_filter_and_an_indefinite_start).  Returns the number of steps compared."""
    T = ref['m'].shape[0]
    f_dev, f_ora = int(got['fn'][b]), first_bad(ref)
    upto = min(f if f >= 0 else T for f in (f_dev, f_ora))
    completed = ref.get('completed', -1)
    if 0 <= completed < upto:
        assert_state(got, b, ref, mi, completed, RTOL, tag)
        return completed
    assert_state(got, b, ref, mi, upto, RTOL, tag)
    if f_dev < 0 and f_ora < 0:
        assert abs(got['nell'][b] - ref['nell']) <= RTOL * abs(ref['nell']), f'{tag}: nell {got["nell"][b]} vs {ref["nell"]}'
    elif f_dev >= 0:
        assert np.isnan(got['nell'][b]) and np.all(np.isnan(got['m'][b, f_dev:])), tag
    if f_dev != f_ora:
        later = got['m'][b] if (f_ora >= 0 and (f_dev < 0 or f_dev > f_ora)) else ref['m']
        conds = [np.linalg.cond(later[t][inds[0]]) for t in range(max(upto - 2, 0), min(upto + 1, T))
                 if np.all(np.isfinite(later[t]))]
        assert conds and max(conds) >= 1e13, \
            f'{tag}: poisons at step {f_dev} (device) / {f_ora} (oracle), cond {max(conds, default=0.):.1e}'
    return upto


# ---- likelihoods from a factor spec -------------------------------------------------------------------------------------
# A likelihood is a list of factors (kind, component, y-column, parameter): 'gaussian' N(y; x, p^2), 'poisson' with rate
# softplus(p x), 'bernoulli' with probability logistic(p x - 1).  KIND_NAMES: what the tracer calls each kind.
KIND_NAMES = {'gaussian': 'gaussian', 'poisson': 'poisson_softplus', 'bernoulli': 'bernoulli_logistic'}


def _factor(kind, y, xk, p, dev):
    if kind == 'gaussian':
        return stats.norm_pdf(y, xk, p) if dev else om.norm_pdf(y, xk, p)
    if kind == 'poisson':
        return stats.poisson_pmf(y, sym.log(1. + sym.exp(xk * p))) if dev else om.poisson_pmf(y, np.log1p(np.exp(xk * p)))
    return (stats.bernoulli_pmf(y, 1. / (1. + sym.exp(-(xk * p) + 1.))) if dev else
            om.bernoulli_pmf(y, 1. / (1. + np.exp(-(xk * p) + 1.))))


def factor_pdfs(spec):
    """-> (device pdf, oracle pdf): the product of the factors of `spec` in that order; y is indexed by column."""
    def pdf(y, x):
        return math.prod(_factor(kind, y[c], x[j], p, True) for kind, j, c, p in spec)

    def opdf(y, x):
        return float(math.prod(_factor(kind, y[c], x[j], p, False) for kind, j, c, p in spec))
    return pdf, opdf
