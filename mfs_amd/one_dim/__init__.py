"""1-D moment filters and their post-processing, mirroring `mfs.one_dim`."""
from mfs_amd.one_dim.moments import cf_errors, characteristic_fn, characteristic_from_pdf

__all__ = ['cf_errors', 'characteristic_fn', 'characteristic_from_pdf']
