"""Measurement models (the jax.scipy.stats calls of the reference's models): numeric on arrays, and a device
`LikelihoodSpec` when traced with the placeholders of `mfs_amd.sym`.  At d = 3 an argument that reads several state
components (a polynomial, its sqrt, an arctan2) gives a `JointLikelihoodSpec`."""
import math

import numpy as np
import scipy.special

from mfs_amd import sym


def _ycol(y):
    return getattr(y, 'ycol', None) or 0


def _vectorised(fn, y, arg, *rest):
    """Elementwise likelihood on a vector of symbolic states: entry k pairs y[k] with arg[k]."""
    if isinstance(arg, (list, tuple, np.ndarray)) and len(arg) and any(sym.is_symbolic(v) for v in np.ravel(arg)):
        arg = list(np.ravel(arg))
        ys = [y[k] for k in range(len(arg))] if isinstance(y, sym._Measurement) and y.ycol is None else [y] * len(arg)
        rests = [[r[k] if isinstance(r, (list, tuple, np.ndarray)) and np.ndim(r) else r for r in rest]
                 for k in range(len(arg))]
        return sym.LikelihoodVector([fn(ys[k], arg[k], *rests[k]) for k in range(len(arg))])
    return None


def _is_joint_arg(u):
    return isinstance(u, sym._JointLink) or sym._is_joint_poly(u)


def batch_likelihoods(per_replicate):
    """Stack B measurement models of one structure (one per replicate: sensor positions, noise levels) into one whose factor
    parameters and joint coefficient blocks carry a leading replicate axis -- the likelihood counterpart of
    `mfs_amd.multi_dims.moments.batch_closures`.  The filters then need `ys` with a leading replicate axis of length B."""
    per_replicate = list(per_replicate)

    def stacked(y, x):
        traced = []
        for fn in per_replicate:
            spec = fn(y, x)
            if isinstance(spec, sym.LikelihoodVector):
                spec = spec.prod()
            if not isinstance(spec, (sym.LikelihoodSpec, sym.LikelihoodProduct)):
                raise sym.NotDeviceDescribable('batch_likelihoods: every member must trace to a device likelihood')
            traced.append(spec.factors)
        out = []
        for fs in zip(*traced):
            first = fs[0]
            key = lambda f: (type(f), f.kind, getattr(f, 'link', None), int(f.component), f.ycol)   # noqa: E731
            if any(key(f) != key(first) for f in fs) or len({len(t) for t in traced}) != 1:
                raise sym.NotDeviceDescribable('batch_likelihoods: the members must have the same factors in the same order '
                                               '(kind, link, component, measurement column)')
            if any(np.asarray(f.params).ndim != 1 for f in fs):
                raise sym.NotDeviceDescribable('batch_likelihoods: the members must not be batched themselves')
            if isinstance(first, sym.JointLikelihoodSpec):
                E = max(f.coef.shape[-1] for f in fs)
                coef = np.zeros((len(fs), 2, E, E, E))
                for b, f in enumerate(fs):
                    e = f.coef.shape[-1]
                    coef[b, :, :e, :e, :e] = f.coef
                out.append(sym.JointLikelihoodSpec(first.kind, first.link, coef, np.stack([f.params[0] for f in fs]),
                                                   first.ycol))
            else:
                out.append(sym.LikelihoodSpec(first.kind, np.stack([f.params for f in fs]), first.component, first.ycol))
        return out[0] if len(out) == 1 else sym.LikelihoodProduct(out)

    return stacked


def bernoulli_pmf(y, p):
    """jax.scipy.stats.bernoulli.pmf(y, p) (mfs/one_dim/ss_models.py:46-47, mfs/multi_dims/ss_models.py:66-67)."""
    vec = _vectorised(bernoulli_pmf, y, p)
    if vec is not None:
        return vec
    if isinstance(p, sym._Logistic) and _is_joint_arg(p.z):
        return sym.joint_spec('bernoulli_logistic', p.z, 0., _ycol(y))
    if isinstance(p, sym._Logistic):
        z = p.z.trimmed()
        if z.umap not in (None, 'x') or z.degree > 3:
            raise sym.NotDeviceDescribable('Bernoulli likelihood: logistic of a polynomial in x of degree <= 3')
        return sym.LikelihoodSpec('bernoulli_logistic', sym._pad(z.coef, 3), component=z.comp or 0, ycol=_ycol(y))
    if sym.is_symbolic(p) or sym.is_symbolic(y):
        raise sym.NotDeviceDescribable('bernoulli_pmf: p must be 1 / (1 + exp(-poly(x)))')
    y = np.asarray(y, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(all='ignore'):
        return np.exp(scipy.special.xlogy(y, p) + scipy.special.xlog1py(1. - y, -p))


def poisson_pmf(y, rate):
    """jax.scipy.stats.poisson.pmf(y, rate) (mfs/one_dim/ss_models.py:83-84)."""
    vec = _vectorised(poisson_pmf, y, rate)
    if vec is not None:
        return vec
    if isinstance(rate, sym._Softplus) and _is_joint_arg(rate.q):
        return sym.joint_spec('poisson_softplus', rate.q, 0., _ycol(y))
    if isinstance(rate, sym._Softplus):
        q = rate.q.trimmed()
        if q.umap not in (None, 'x') or q.degree > 1 or np.any(sym._pad(q.coef, 1)[..., 0] != 0.):
            raise sym.NotDeviceDescribable('Poisson likelihood: rate must be log(1 + exp(l * x))')
        return sym.LikelihoodSpec('poisson_softplus', sym._pad(q.coef, 1)[..., 1:2], component=q.comp or 0, ycol=_ycol(y))
    if sym.is_symbolic(rate) or sym.is_symbolic(y):
        raise sym.NotDeviceDescribable('poisson_pmf: rate must be log(1 + exp(l * x))')
    y = np.asarray(y, dtype=np.float64)
    rate = np.asarray(rate, dtype=np.float64)
    with np.errstate(all='ignore'):
        return np.exp(scipy.special.xlogy(y, rate) - scipy.special.gammaln(y + 1.) - rate)


def norm_pdf(y, loc, scale):
    """jax.scipy.stats.norm.pdf(y, loc, scale) (dardel/convergence/convergence_mf.py:58-61)."""
    vec = _vectorised(norm_pdf, y, loc, scale)
    if vec is not None:
        return vec
    if isinstance(loc, sym._Bearing):     # y ~ N(arctan2(x[1], x[0]), scale^2): a factor of both state components (component 2)
        var = np.asarray(scale, dtype=sym._DTYPE[0]) ** 2
        return sym.LikelihoodSpec('bearing_gaussian', var[..., None], component=2, ycol=_ycol(y))
    if _is_joint_arg(loc):                # d = 3: y ~ N(u(x), scale^2), u a polynomial / sqrt / arctan2 of all components
        if np.ndim(scale) != 0:
            raise sym.NotDeviceDescribable('per-replicate noise levels of a joint likelihood factor: trace one measurement '
                                           'model per replicate and stack them with mfs_amd.stats.batch_likelihoods')
        return sym.joint_spec('gaussian', loc, float(scale) ** 2, _ycol(y))
    if isinstance(loc, sym.Poly):
        q = loc.trimmed()
        if q.umap not in (None, 'x') or q.degree > 1:
            raise sym.NotDeviceDescribable('Gaussian likelihood: loc must be l0 * x + l1')
        c = sym._pad(q.coef, 1)
        var = np.asarray(scale, dtype=sym._DTYPE[0]) ** 2
        lead = np.broadcast_shapes(c.shape[:-1], var.shape)      # per-replicate loc coefficients and / or scale
        c, var = np.broadcast_to(c, lead + (2,)), np.broadcast_to(var, lead)
        return sym.LikelihoodSpec('gaussian', np.stack([c[..., 1], c[..., 0], var], axis=-1), component=q.comp or 0,
                                  ycol=_ycol(y))
    if sym.is_symbolic(loc) or sym.is_symbolic(y):
        raise sym.NotDeviceDescribable('norm_pdf: loc must be l0 * x + l1')
    with np.errstate(all='ignore'):
        return np.exp(-0.5 * ((np.asarray(y) - loc) / scale) ** 2) / (math.sqrt(2 * math.pi) * scale)
