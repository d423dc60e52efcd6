"""Classical filters, mirroring `mfs.classical_filters_smoothers`: the brute-force grid filter (the ground truth the moment
filters are measured against), the bootstrap particle filter with stratified / systematic resampling (d = 1, 2), and the
Gaussian filters -- the sigma-point filter `sgp_filter` with the Gauss--Hermite and cubature rules of `SigmaPoints`, and the
extended Kalman filter `ekf` -- for d = 1, 2: the competitors of the paper's tables.  The smoothers, the continuous-discrete
filters, `kf` and the optimal-proposal particle filter of the reference's package are not here."""
from mfs_amd.classical_filters_smoothers import resampling
from mfs_amd.classical_filters_smoothers.resampling import stratified, systematic, multinomial
from mfs_amd.classical_filters_smoothers.smc import (bootstrap_filter, gaussian_transition, ParticleFilterResult,
                                                     ParticleFilterResultND)
from mfs_amd.classical_filters_smoothers.quadratures import SigmaPoints
from mfs_amd.classical_filters_smoothers.gfs import sgp_filter, ekf, gaussian_transition_nd, measurement_moments

__all__ = ['bootstrap_filter', 'gaussian_transition', 'ParticleFilterResult', 'ParticleFilterResultND', 'resampling',
           'stratified', 'systematic', 'multinomial', 'SigmaPoints', 'sgp_filter', 'ekf', 'gaussian_transition_nd',
           'measurement_moments']
