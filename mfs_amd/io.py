"""On-disk result format of the reference's drivers, so that
`reproduce_paper_plots/*.py` and the post-processing scripts consume this build's outputs unchanged.

Keys (dardel/benes_bernoulli/mf.py:83-92): raw -> rmss, nell; central -> cmss, means, nell; scaled -> scmss, means,
scales, nell.  One file per Monte-Carlo run `{mode}{_normal}_N_{N}_mc_{k}.npz` (mf.py:82)."""
import os

import numpy as np

_KEYS = {'raw': ('rmss', 'nell'), 'central': ('cmss', 'means', 'nell'), 'scaled': ('scmss', 'means', 'scales', 'nell')}


def result_filename(directory, mode, N, k, normal=False):
    return os.path.join(directory, f"{mode}{'_normal' if normal else ''}_N_{N}_mc_{k}.npz")


def save_filter_result(filename, mode, *arrays):
    """`arrays` in the order the filter returns them, for ONE replicate."""
    keys = _KEYS[mode]
    if len(arrays) != len(keys):
        raise ValueError(f'{mode} mode stores {keys}, got {len(arrays)} arrays')
    np.savez_compressed(filename, **dict(zip(keys, arrays)))


def save_batch(directory, mode, N, arrays, normal=False, first_k=0):
    """Split batched filter outputs (leading replicate axis) into the reference's one-file-per-run layout."""
    os.makedirs(directory, exist_ok=True)
    B = np.asarray(arrays[-1]).shape[0]
    for b in range(B):
        save_filter_result(result_filename(directory, mode, N, first_k + b, normal), mode, *[np.asarray(a)[b] for a in arrays])
    return B


def load_filter_result(filename, mode):
    data = np.load(filename)
    return tuple(data[k] for k in _KEYS[mode])


def save_pf_result(filename, means, cfs):
    """One particle-filter run in the layout dardel/benes_bernoulli/pf.py:74-75 writes: the filtering means (T,) and the
    empirical characteristic functions (T, nz) of its samples."""
    np.savez_compressed(filename, pf_filtering_means=np.asarray(means), pf_filtering_cfs=np.asarray(cfs))


def load_pf_result(filename):
    data = np.load(filename)
    return data['pf_filtering_means'], data['pf_filtering_cfs']


def save_pf_errs(filename, errs):
    """One 2-D particle-filter run in the layout dardel/prey_predator/pf.py:77 writes: the absolute errors (T, 2) of the
    filtering means against the simulated trajectory, under the key `errs`."""
    np.savez_compressed(filename, errs=np.asarray(errs))


def load_pf_errs(filename):
    return np.load(filename)['errs']


def save_brute_force_summary(filename, true_trajs, true_filtering_means, true_filtering_cfs):
    """The packed ground truth dardel/benes_bernoulli/post_processing_brute_force.py:53-55 writes and compute_errs.py:39-44
    reads: the simulated trajectories (runs, T), the grid filter's means (runs, T) and the characteristic functions of its
    posteriors (runs, T, m) complex128."""
    np.savez_compressed(filename, true_trajs=np.asarray(true_trajs), true_filtering_means=np.asarray(true_filtering_means),
                        true_filtering_cfs=np.asarray(true_filtering_cfs))


def load_brute_force_summary(filename):
    data = np.load(filename)
    return data['true_trajs'], data['true_filtering_means'], data['true_filtering_cfs']


# the sixteen arrays of dardel/benes_bernoulli/compute_errs.py:115-128, in its order
BENES_BERNOULLI_ERR_KEYS = (
    'true_trajs_vs_true_means_abs', 'true_trajs_vs_mf_means_abs', 'true_trajs_vs_ghf_means_abs', 'true_trajs_vs_pf_means_abs',
    'true_means_vs_mf_means_abs', 'true_means_vs_ghf_means_abs', 'true_means_vs_pf_means_abs',
    'true_cfs_vs_mf_l1', 'true_cfs_vs_mf_l2', 'true_cfs_vs_mf_sup',
    'true_cfs_vs_ghf_l1', 'true_cfs_vs_ghf_l2', 'true_cfs_vs_ghf_sup',
    'true_cfs_vs_pf_l1', 'true_cfs_vs_pf_l2', 'true_cfs_vs_pf_sup')


def save_benes_bernoulli_errs(filename, **errs):
    """The error file of dardel/benes_bernoulli/compute_errs.py:115-128: exactly its sixteen keys, each given by name."""
    if set(errs) != set(BENES_BERNOULLI_ERR_KEYS):
        missing, extra = set(BENES_BERNOULLI_ERR_KEYS) - set(errs), set(errs) - set(BENES_BERNOULLI_ERR_KEYS)
        raise ValueError(f'the error file has the keys {BENES_BERNOULLI_ERR_KEYS}; missing {sorted(missing)}, '
                         f'unknown {sorted(extra)}')
    np.savez_compressed(filename, **{k: np.asarray(errs[k]) for k in BENES_BERNOULLI_ERR_KEYS})
