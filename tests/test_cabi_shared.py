"""The shared-graph lattice entry points of the C ABI (include/asr_amd.h,
asr_lattice_shared_*): declared, exported, bound, and checking their arguments without a GPU."""
import ctypes

from test_cabi import _declared

SHARED = ['asr_lattice_shared_forward_f32', 'asr_lattice_shared_fwbw_f32',
          'asr_lattice_shared_supported', 'asr_lattice_shared_workspace_bytes']


def test_shared_entry_points_are_declared_exported_and_bound():
    from att_speech import _native
    assert [n for n in _declared() if n.startswith('asr_lattice_shared_')] == SHARED
    handle = ctypes.CDLL(_native.LIB_PATH)
    for n in SHARED:
        assert hasattr(handle, n), n
        assert n in _native._SIGNATURES
    # additions only: the version every binding checks is unchanged
    assert _native.lib().asr_abi_version() == _native.ABI_VERSION == 24


def test_shared_argument_checks_need_no_gpu():
    from att_speech import _native
    L = _native.lib()
    assert L.asr_lattice_shared_supported(196, 7690, 49) == 1
    assert L.asr_lattice_shared_supported(2054, 156650, 49) == 1      # mono CTC o trigram LM
    assert L.asr_lattice_shared_supported(7169, 10, 49) == 0
    assert L.asr_lattice_shared_supported(100, 10, 2401) == 0         # bigram-context classes
    assert L.asr_lattice_shared_workspace_bytes(10, 2, 7) >= 10 * 2 * 7 * 4
    assert L.asr_lattice_shared_workspace_bytes(-1, 2, 7) == -1
    nul = [None] * 6
    # null pointers, lanes that are no power of two, a sign other than +-1
    assert L.asr_lattice_shared_fwbw_f32(None, 4, 2, 5, None, 3, 4, *nul, 3, 1, None, 3, 1, -1e20, 1.0, 0,
                                         None, None, None, None, 0, None) == _native.ASR_EINVAL
    assert L.asr_lattice_shared_fwbw_f32(None, 4, 2, 5, None, 3, 4, *nul, 3, 3, None, 3, 1, -1e20, 1.0, 0,
                                         None, None, None, None, 0, None) == _native.ASR_EINVAL
    assert L.asr_lattice_shared_fwbw_f32(None, 4, 2, 5, None, 3, 4, *nul, 3, 1, None, 3, 1, -1e20, 0.5, 0,
                                         None, None, None, None, 0, None) == _native.ASR_EINVAL
    assert L.asr_lattice_shared_fwbw_f32(None, 4, 0, 5, None, 3, 4, *nul, 3, 1, None, 3, 1, -1e20, 1.0, 0,
                                         None, None, None, None, 0, None) == _native.ASR_OK
    assert L.asr_lattice_shared_fwbw_f32(None, 4, 2, 2401, None, 3, 4, *nul, 3, 1, None, 3, 1, -1e20, 1.0, 0,
                                         None, None, None, None, 0, None) == _native.ASR_EUNSUPPORTED
    assert L.asr_lattice_shared_forward_f32(None, 4, 2, 5, None, 3, 4, None, None, None, None, 3, 1, -1e20, 1,
                                            None, None, None, 0, None) == _native.ASR_EINVAL
