"""Classical filters, mirroring `mfs.classical_filters_smoothers`: the brute-force grid filter (the ground truth the moment
filters are measured against) and the bootstrap particle filter with stratified / systematic resampling (the competitor of the
paper's 1-D tables).  The Gaussian filters and the optimal-proposal particle filter of the reference's package are not here."""
from mfs_amd.classical_filters_smoothers import resampling
from mfs_amd.classical_filters_smoothers.resampling import stratified, systematic, multinomial
from mfs_amd.classical_filters_smoothers.smc import bootstrap_filter, gaussian_transition, ParticleFilterResult

__all__ = ['bootstrap_filter', 'gaussian_transition', 'ParticleFilterResult', 'resampling', 'stratified', 'systematic',
           'multinomial']
