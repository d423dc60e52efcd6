"""The include layers of mfs_amd/csrc: device code that several kernel families use lives in the shared headers, no kernel
header includes another family's, and the host layer (capi.hip and the capi_*.hip units, one per filter family) includes no
kernel header at all.

For every translation unit of csrc/Makefile the preprocessor lists what it reaches (`hipcc -MM`, no compilation); the
project headers among them must be the unit's own family's kernel headers plus the shared layer.  No GPU and no library."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mfs_amd', 'csrc')

# owned by no kernel family: any unit may reach these
SHARED = {'device_util.hpp', 'likelihood.hpp', 'kernel_args.hpp', 'particle_stream.hpp', 'registry.hpp', 'launch_util.hpp'}
# the host layer's own
HOST_ONLY = {'staging.hpp', 'pool.hpp', 'host_run.hpp'}
# the host units: the core of the C ABI and one unit per filter family
HOST_UNITS = {'capi.hip', 'capi_1d.hip', 'capi_nd.hip', 'capi_grid.hip', 'capi_classical.hip'}
# the 1-D fast kernel runs the dense `quadrature` in place (its extended variant), so the two headers are one family
FAST_1D = {'filter1d_fast.hpp', 'filter1d_kernel.hpp'}
# unit -> (the -D set of one of its Makefile rules, the kernel headers of its family)
UNITS = {
    **{unit: ([], set()) for unit in HOST_UNITS},
    'filter1d_inst.hip': (['-DMFS_NLO=14', '-DMFS_NHI=16'], FAST_1D),
    'filter1d_spec_inst.hip': (['-DMFS_SPEC_N=15'], FAST_1D),
    'filter1d_partner_inst.hip': (['-DMFS_SPEC_N=15'], FAST_1D | {'filter1d_partner.hpp'}),
    'filter1d_grad_inst.hip': ([], {'filter1d_grad.hpp'}),
    # the d = 2 kernel uses the DPP broadcast and lane-swap helpers that stay with the 1-D fast kernel
    'filternd_inst.hip': ([], FAST_1D | {'filternd_kernel.hpp'}),
    'filternd3_inst.hip': ([], {'filternd3_kernel.hpp'}),
    'gridfilter_inst.hip': ([], {'gridfilter_kernel.hpp'}),
    'particle_inst.hip': ([], {'particle_kernel.hpp'}),
    'particle_nd_inst.hip': ([], {'particle_nd_kernel.hpp'}),
    'gaussfilter_inst.hip': ([], {'gaussfilter_kernel.hpp'}),
    # the diagnostic of the shared layer itself: no family
    'device_math_inst.hip': ([], set()),
}


def _hipcc():
    for cand in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and os.path.isfile(cand) and os.access(cand, os.X_OK):
            return cand
    return None


HIPCC = _hipcc()
pytestmark = pytest.mark.skipif(HIPCC is None, reason='no hipcc: the preprocessor is the one of the build')


def _reached(unit, defines):
    """Names of the csrc headers the unit's preprocessing reaches (host and device pass together)."""
    out = subprocess.run([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-I' + os.path.join(ROOT, 'include'), *defines, '-MM',
                          os.path.join(CSRC, unit)], check=True, capture_output=True, text=True).stdout
    paths = {os.path.realpath(tok) for tok in out.replace('\\\n', ' ').split() if tok.endswith('.hpp')}
    assert paths, out
    return {os.path.basename(p) for p in paths if os.path.dirname(p) == os.path.realpath(CSRC)}


def test_every_translation_unit_is_listed():
    on_disk = {os.path.basename(p) for p in glob.glob(os.path.join(CSRC, '*.hip'))}
    assert on_disk == set(UNITS)
    headers = {os.path.basename(p) for p in glob.glob(os.path.join(CSRC, '*.hpp'))}
    assert SHARED | HOST_ONLY <= headers
    for _, family in UNITS.values():
        assert family <= headers - SHARED - HOST_ONLY


@pytest.mark.parametrize('unit', sorted(UNITS))
def test_unit_reaches_only_its_family_and_the_shared_layer(unit):
    defines, family = UNITS[unit]
    reached = _reached(unit, defines)
    if unit in HOST_UNITS:
        # the host layer: launchers and argument structs through registry.hpp, no device code
        assert reached == {'registry.hpp', 'kernel_args.hpp'} | HOST_ONLY
    else:
        assert not reached & HOST_ONLY
        assert reached - SHARED == family
