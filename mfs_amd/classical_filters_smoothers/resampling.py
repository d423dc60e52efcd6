"""Resampling schemes of the device particle filter, mirroring the names of `mfs.classical_filters_smoothers.resampling`.

The reference's resamplers are functions (weights, key) -> indices that draw from JAX keys; on the device the resampling runs
inside the filter's kernels from its own counter-based stream (include/mfs_hip.h), so the names here are descriptors that
`bootstrap_filter` takes in the `resampling` slot.  `stratified` and `systematic` (resampling.py:43-59) are built;
`multinomial` is named so that asking for it fails with a message instead of an AttributeError.
"""
from typing import NamedTuple, Optional

__all__ = ['Resampling', 'stratified', 'systematic', 'multinomial']


class Resampling(NamedTuple):
    name: str
    code: Optional[int]   # MFS_RESAMPLE_* of include/mfs_hip.h, None if the device has no such scheme


stratified = Resampling('stratified', 0)      # one uniform per particle: target (i + u_i) / n
systematic = Resampling('systematic', 1)      # one uniform for all: target (i + u) / n
multinomial = Resampling('multinomial', None)
