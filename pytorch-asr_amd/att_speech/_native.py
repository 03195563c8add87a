"""ctypes binding of libasr_amd.so (include/asr_amd.h) for torch tensors.

PyTorch is used here only as the owner of device memory and streams: every
function takes CUDA(ROCm) tensors, passes raw device pointers + sizes + the
current HIP stream through the C ABI, and returns tensors it allocated with
torch.  There is NO CPU or eager fallback: a missing library or a non-GPU tensor
raises immediately.
"""
import ctypes
import warnings
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get(     # ASR_AMD_LIB: development override (kernel A/B builds)
    'ASR_AMD_LIB', os.path.join(os.path.dirname(_HERE), 'csrc', 'libasr_amd.so'))

ASR_OK, ASR_EINVAL, ASR_EUNSUPPORTED, ASR_ELAUNCH = 0, 1, 2, 3
ABI_VERSION = 24

_lib = None
# bench.py sets this to a list to collect (start, end) torch.cuda.Event pairs
# around every lattice forward-backward call (launched on the current stream)
EVENT_HOOK = None
_WARNED = {}

_vp, _i, _i64, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float

# the LM of asr_lattice_lmrescore_*: states, arcs, six CSR / back-off arrays, start, label map and length, oov cost
_LM_ARGS = [_i64, _i64] + [_vp] * 6 + [_i, _vp, _i64, ctypes.c_double]
# DeviceLatticeBatch._common_args, shared by the six lattice DP launches: nodes, arcs, levels and the batch's 21
# arrays; after the two scales the graph's states, arcs, three arrays and start, and the threads a workgroup
_LAT_HEAD = [_i64, _i64, _i64] + [_vp] * 21
_LAT_TAIL = [_i64, _i64] + [_vp] * 3 + [_i, _i]
_LAT_SCALES = [ctypes.c_double] * 2
_WS = [_vp, _i64, _vp]          # workspace, its bytes, stream

_SIGNATURES = {
    'asr_abi_version': (ctypes.c_int, []),
    'asr_strerror': (ctypes.c_char_p, [_i]),
    'asr_lattice_fwbw_workspace_bytes': (_i64, [_i, _i, _i, _i]),
    'asr_lattice_fwbw_f32': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp,
                                  _vp, _i64, _vp]),
    'asr_lattice_fwbw_signed_f32': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp,
                                         _vp, _i64, _vp]),
    'asr_scale_rows_f32': (_i, [_vp, _i, _i, _i, _vp, _vp]),
    'asr_lattice_fwbw_band_supported': (_i, [_i] * 7),
    'asr_lattice_fwbw_band_f32': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp,
                                       _vp, _i64, _vp, _vp, _vp, _i, _vp]),
    'asr_lattice_viterbi_workspace_bytes': (_i64, [_i, _i, _i]),
    'asr_lattice_forward_f32': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp,
                                     _i, _i, _i, _f, _i, _vp, _vp, _vp, _i64,
                                     _vp]),
    'asr_log_softmax_fwd_f32': (_i, [_vp, _i64, _i, _vp, _vp]),
    'asr_log_softmax_bwd_f32': (_i, [_vp, _vp, _i64, _i, _vp, _vp]),
    'asr_sub_rowmax_f32': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    'asr_argmax_rows_f32': (_i, [_vp, _i64, _i, _vp, _vp]),
    'asr_conv7x7c32_workspace_bytes': (_i64, []),
    'asr_conv7x7c32_supported': (_i, [_i, _i, _i, _i]),
    'asr_conv1_7x7s2_supported': (_i, [_i, _i]),
    'asr_conv7x7c32_fwd_bf16': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i64, _vp]),
    'asr_conv7x7c32_bwd_data_bf16': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i64, _vp]),
    'asr_conv7x7c32_wgrad_bf16': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i64, _vp]),
    'asr_conv1_7x7s2_workspace_bytes': (_i64, []),
    'asr_conv1_7x7s2_fwd': (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i64, _vp]),
    'asr_conv1_7x7s2_wgrad': (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i64, _vp]),
    'asr_conv1_7x7s2_wgrad_bn_supported': (_i, [_i]),
    'asr_conv1_7x7s2_wgrad_bn': (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _f,
                                      _vp, ctypes.c_double, _vp, _vp, _i64, _vp]),
    'asr_conv1c_7x7s2_workspace_bytes': (_i64, [_i]),
    'asr_conv1c_7x7s2_fwd': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i64, _vp]),
    'asr_conv1c_7x7s2_wgrad': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i64, _vp]),
    'asr_log_softmax_shift_fwd_f32': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    'asr_log_softmax_shift_bwd_f32': (_i, [_vp, _vp, _vp, _i64, _i, _vp, _vp]),
    'asr_sum_leading_f32': (_i, [_vp, _i, _i64, _vp, _vp]),
    'asr_adam_chunk_elems': (_i, []),
    'asr_grad_sumsq_partials_f32': (_i, [_vp, _i64, _vp, _i, _vp]),
    'asr_adam_clip_step_f32': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _f, _f, _f, _f, _f, _f, _f,
                                    _vp, _vp, _vp, _vp]),
    'asr_adam_clip_step_ex_f32': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _f, _f, _f, _f, _f, _f, _f,
                                       _vp, _vp, _vp, _vp, _vp]),
    'asr_nonfinite_flag_f32': (_i, [_vp, _i, _vp, _vp]),
    'asr_noise_chunk_elems': (_i, []),
    'asr_gaussian_noise_f32': (_i, [_vp, _i, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, _i, _i, _vp]),
    'asr_edit_distance_max_len': (_i, []),
    'asr_edit_distance_stats_i32': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    'asr_ctc_align_supported': (_i, [_i, _i, _i]),
    'asr_ctc_align_workspace_bytes': (_i64, [_i, _i, _i]),
    'asr_ctc_align_f64': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i,
                               _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'asr_wfst_decode_supported': (_i, [_i64, _i64, _i, _i]),
    'asr_wfst_decode_workspace_bytes': (_i64, [_i64, _i, _i64, _i64]),
    'asr_wfst_decode_f32': (_i, [_vp, _i64, _vp, _i, _i, _i, _i64, _i64] + [_vp] * 9 + [_i64, _vp, _i, _i,
                                 _f, _f, _i, _i64, _i64, _i, _i] + [_vp] * 8 + [_i64, _vp]),
    'asr_wfst_lattice_supported': (_i, [_i64, _i64, _i, _i]),
    'asr_wfst_lattice_workspace_bytes': (_i64, [_i64, _i, _i, _i64, _i64]),
    'asr_wfst_lattice_f32': (_i, [_vp, _i64, _vp, _i, _i, _i, _i64, _i64] + [_vp] * 9 + [_i64, _vp, _i, _i,
                                  _f, _f, _f, _i, _i64, _i64, _i64, _i64, _i] + [_vp] * 14 + [_i64, _vp]),
    'asr_lattice_bestpath_supported': (_i, [_i64, _i64, _i64]),
    'asr_lattice_bestpath_workspace_bytes': (_i64, [_i64, _i]),
    'asr_lattice_bestpath_f64': (_i, [_i] * 4 + _LAT_HEAD + [_vp] * 2 + _LAT_TAIL + [_vp] * 4 + _WS),
    'asr_lattice_posterior_supported': (_i, [_i64, _i64, _i64]),
    'asr_lattice_posterior_workspace_bytes': (_i64, [_i64]),
    'asr_lattice_posterior_f64': (_i, [_i] * 3 + _LAT_HEAD + _LAT_SCALES + _LAT_TAIL + [_vp] * 4 + _WS),
    'asr_lattice_nbest_supported': (_i, [_i64, _i64, _i64, _i]),
    'asr_lattice_nbest_workspace_bytes': (_i64, [_i64, _i]),
    'asr_lattice_nbest_f64': (_i, [_i] * 4 + _LAT_HEAD + _LAT_SCALES + _LAT_TAIL + [_vp] * 5 + _WS),
    'asr_lattice_mbr_supported': (_i, [_i64, _i64, _i64, _i]),
    'asr_lattice_mbr_workspace_bytes': (_i64, [_i64, _i]),
    'asr_lattice_mbr_f64': (_i, [_i] * 3 + _LAT_HEAD + _LAT_SCALES + _LAT_TAIL + [_vp] * 4 + [_i, _i, _i64] +
                            [_vp] * 11 + _WS),
    'asr_lattice_oracle_supported': (_i, [_i64, _i64, _i64, _i]),
    'asr_lattice_oracle_workspace_bytes': (_i64, [_i64, _i]),
    'asr_lattice_oracle_i32': (_i, [_i] * 3 + _LAT_HEAD + _LAT_SCALES + _LAT_TAIL + [_vp] * 2 + [_i] + [_vp] * 7 + _WS),
    'asr_lattice_seqtrain_supported': (_i, [_i64, _i64, _i64]),
    'asr_lattice_seqtrain_workspace_bytes': (_i64, [_i64]),
    'asr_lattice_seqtrain_f64': (_i, [_i] * 3 + _LAT_HEAD + _LAT_SCALES + _LAT_TAIL + [_vp] * 2 + [_i, _i, _vp, _i,
                                 ctypes.c_double, _i64, _i64] + [_vp] * 8 + _WS),
    'asr_lattice_lmrescore_supported': (_i, [_i64, _i64, _i64, _i]),
    'asr_lattice_lmrescore_workspace_bytes': (_i64, [_i64, _i]),
    'asr_lattice_lmrescore_expand': (_i, [_i] * 4 + [_i64] * 3 + [_vp] * 11 + [_i64, _vp, _i] + _LM_ARGS + [_vp] * 3 +
                                     [_i64, _vp]),
    'asr_lattice_lmrescore_emit': (_i, [_i] * 4 + [_i64] * 2 + [_vp] * 8 + [_i64] + [_vp] * 2 + _LM_ARGS +
                                   [ctypes.c_double] + [_vp] * 3 + [_i64] * 2 + [_vp] * 9 + [_i64, _vp]),
    'asr_lattice_lmrescore_sweep': (_i, [_i] + [_i64] * 4 + [_vp] * 18 + [_i64, _vp, _i, _i64, _vp, _i,
                                    ctypes.c_double, ctypes.c_double, _i] + [_vp] * 6),
    'asr_split_bf16_f32': (_i, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp]),
    'asr_log_softmax_shift_bwd_split_blocks': (_i, [_i64]),
    'asr_log_softmax_shift_bwd_split_bf16': (_i, [_vp, _vp, _vp, _i64, _i, _vp, _vp, _i, _vp, _vp]),
    'asr_tcn_attention_step_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp,
                                        _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    'asr_tcn_attention_step_win_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp,
                                            _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    'asr_tcn_attention_scan_fwd_f32': (_i, [_vp] * 6 + [_f, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    'asr_tcn_attention_scan_bwd_f32': (_i, [_vp] * 5 + [_f, _vp, _vp, _vp, _i, _i, _i, _i, _i] +
                                       [_vp] * 6),
    'asr_att_gru_scan_fwd_f32': (_i, [_vp] * 11 + [_i] * 7 + [_vp] * 6),
    'asr_att_gru_scan_bwd_f32': (_i, [_vp] * 14 + [_i] * 6 + [_vp] * 7),
    'asr_beam_step_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f,
                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'asr_beam_lm_supported': (_i, [_i, _i, _i]),
    'asr_lm_label_costs_f64': (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp]),
    'asr_lm_bag_advance_f64': (_i, [_vp] * 6 + [_i, _i] + [_vp] * 7 + [_i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    'asr_beam_lm_step_f32': (_i, [_vp, _vp, _vp, _vp, ctypes.c_double] + [_vp] * 7 + [_i] * 6 +
                             [_f, ctypes.c_double, _f, _f] + [_vp] * 15),
    'asr_graph_search_supported': (_i, [_i, _i, _i, _i]),
    'asr_beam_lm_step_graph_f32': (_i, [_vp, _vp, _vp, _vp, ctypes.c_double] + [_vp] * 7 + [_i] * 6 +
                                   [_f, ctypes.c_double, _f, _f] + [_vp] * 17),
    'asr_graph_merge_f32': (_i, [_vp] * 9 + [_i, _vp, _vp] + [_i] * 6 + [_f, _i] + [_vp] * 10),
    'asr_forced_level_f32': (_i, [_vp] * 11 + [_i] * 8 + [_f, _vp, _vp, _vp]),
    'asr_ctc_graph_build': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _f] + [_vp] * 8),
    'asr_lattice_grouped_workspace_bytes': (_i64, [_i, _i, _i, _i]),
    'asr_lattice_grouped_fwbw_f32': (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _i] + [_vp] * 8 +
                                     [_f, _vp, _vp, _vp, _vp, _i64, _vp]),
    'asr_lattice_grouped_fwbw_acc_f32': (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _i] + [_vp] * 8 +
                                         [_f, _i, _vp, _vp, _vp, _vp, _i64, _vp]),
    'asr_lattice_grouped_forward_f32': (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _i] + [_vp] * 8 +
                                        [_f, _i, _vp, _vp, _vp, _i64, _vp]),
    'asr_lattice_shared_supported': (_i, [_i, _i, _i]),
    'asr_lattice_shared_workspace_bytes': (_i64, [_i, _i, _i]),
    'asr_lattice_shared_fwbw_f32': (_i, [_vp, _i, _i, _i, _vp, _i, _i] + [_vp] * 6 + [_i, _i, _vp, _i, _i,
                                         _f, _f, _i, _vp, _vp, _vp, _vp, _i64, _vp]),
    'asr_lattice_shared_forward_f32': (_i, [_vp, _i, _i, _i, _vp, _i, _i] + [_vp] * 4 +
                                       [_i, _i, _f, _i, _vp, _vp, _vp, _i64, _vp]),
    'asr_lstm_workspace_bytes': (_i64, [_i, _i]),
    'asr_lstm_bidir_fwd_bf16': (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    'asr_lstm_bidir_bwd_bf16': (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    'asr_lstm_fused_supported': (_i, [_i, _i, _i]),
    'asr_lstm_wgrad_supported': (_i, [_i]),
    'asr_lstm_dgrad_supported': (_i, [_i]),
    'asr_lstm_dgrad_bf16': (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    'asr_lstm_wgrad_workspace_bytes': (_i64, [_i, _i, _i, _i]),
    'asr_lstm_wgrad_bf16': (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i64, _vp]),
    'asr_lstm_bidir_fwd_fused_bf16': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    'asr_gru_workspace_bytes': (_i64, [_i, _i]),
    'asr_gru_supported': (_i, [_i, _i]),
    'asr_gru_bidir_fwd_bf16': (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    'asr_gru_bidir_bwd_bf16': (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    'asr_bn_act_workspace_bytes': (_i64, [_i]),
    'asr_bn_act_fwd_f32': (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f,
                                _vp, _i, _i, _vp, _vp, _vp, _vp, _i64, _vp]),
    'asr_bn_act_bwd_f32': (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _f, _f,
                                _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'asr_bn_act_bwd_phase_f32': (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _f, _f,
                                      _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i64, _i, ctypes.c_double, _vp]),
    'asr_fbank_supported': (_i, [_i] * 6),
    'asr_fbank_f32': (_i, [_vp, _i64, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f,
                           _vp, _vp, _f, ctypes.c_uint64, ctypes.c_uint64, _vp, _vp, _vp]),
}

class NativeLibraryError(RuntimeError):
    pass


def lib():
    """Load libasr_amd.so; fail loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                "%s is missing: build it with `make -C pytorch-asr_amd/csrc` "
                "(or __graft_entry__.build()); there is no fallback path."
                % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)      # AttributeError if a symbol is missing
            fn.restype = res
            fn.argtypes = args
        if handle.asr_abi_version() != ABI_VERSION:
            raise NativeLibraryError("libasr_amd.so ABI %d != expected %d" % (
                handle.asr_abi_version(), ABI_VERSION))
        _lib = handle
    return _lib


def check(code, what):
    if code == ASR_OK:
        return
    msg = "%s: %s" % (what, lib().asr_strerror(code).decode())
    if code == ASR_EINVAL:
        # the reference raises AssertionError / ValueError on malformed input
        raise AssertionError(msg)
    if code == ASR_EUNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError(msg)


def _dev(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NativeLibraryError(
            "%s must be a GPU tensor: the MI355X path has no CPU fallback" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Graph(object):
    """Device-resident int32/f32 copy of the reference's 4 or 8 padded graph
    matrices (fst_utils.py:222-294,491-521)."""
    __slots__ = ('src_in', 'il_in', 'w_in', 'term', 'dst_out', 'il_out',
                 'w_out', 'Bg', 'N', 'Kin', 'Kout', 'band', 'ctc_labels', 'addend')

    def __init__(self, graph_matrices, device):
        # band: every state n is entered only from {n, n-1, n-2} with weights <= 0 (the CTC
        # chain lattices): lattice_fwbw sends such graphs to asr_lattice_fwbw_band_f32.  Set by
        # build_ctc_graph, or found here on the host when the matrices arrive as CPU tensors
        # (the data workers' hand-over, fst_utils.py:491-521); the kernel re-checks per utterance.
        self.band = False
        self.ctc_labels = None      # (labels [B,Lmax] i32, lens [B] i32) when built from them (order 1)
        # [B] f32 added to every path sum of utterance b, or None: log G(y) of a grammar FST, which
        # weights all alignments of a transcript alike (fst_utils.BaseGraphGen), so the chain lattices
        # stay unweighted and band-shaped
        self.addend = None
        if graph_matrices is None:          # filled in by build_ctc_graph
            return
        gm = list(graph_matrices)
        if len(gm) not in (4, 8):
            raise AssertionError("expected 4 or 8 graph matrices")
        bg = gm[0].size(0)
        if not all(m.size(0) == bg for m in gm):              # fst_utils.py:407
            raise AssertionError("graph matrices disagree on batch size")

        def to_i(m):
            return m.to(device=device, dtype=torch.int32).contiguous()

        def to_f(m):
            return m.to(device=device, dtype=torch.float32).contiguous()
        self.src_in, self.il_in, self.w_in = to_i(gm[0]), to_i(gm[1]), to_f(gm[2])
        self.term = to_f(gm[3]).reshape(bg, -1)
        self.Bg, self.N, self.Kin = self.src_in.shape
        if len(gm) == 8:
            self.dst_out, self.il_out, self.w_out = to_i(gm[4]), to_i(gm[5]), to_f(gm[6])
            self.Kout = self.dst_out.shape[2]
            self.band = _host_band_check(gm)
        else:
            self.dst_out = self.il_out = self.w_out = None
            self.Kout = 0


def _host_band_check(gm):
    """True when the in-arcs of every state n come from {n, n-1, n-2} with weights <= 0
    (CPU tensors only: no device read-back to find out)."""
    src, w = gm[0], gm[2]
    if src.is_cuda or w.is_cuda or src.dim() != 3 or src.size(1) > 256:
        return False
    valid = w > -5e19
    d = torch.arange(src.size(1)).view(1, -1, 1) - src.long()
    return bool(((d >= 0) & (d <= 2) & (w <= 0) | ~valid).all())


# Policy state of the band kernel (csrc/lattice_band.inc): it redoes, inside the launch and ~10x
# slower, the utterances whose numbers leave what a wave-wide scale factor can hold — typically
# ALL utterances of a batch while a CTC model is in its blank-collapse phase (blank ~1, labels
# ~1e-3: alpha peaks at the first states, beta at the last, the paths that matter sit 2^-300
# below both).  The kernel counts them; the count of one call is read (without a sync: pinned
# copy + event) before a later call, and when more than a tenth of a batch was redone the next
# `_BAND_COOLDOWN` calls go to the log-domain kernel, which does not care.
_BAND_STATE = {'cool': 0, 'pending': None, 'launched': 0, 'seen': (0, 0)}
_BAND_COOLDOWN = 64
_BAND_MAX_BATCH = 1 << 30      # no cap: measured faster from 384 utterances up, level with the log-domain kernel below
_BAND_COUNTER = {}             # device -> (running device counter int32[1], pinned host copy)


def _band_counter(device):
    c = _BAND_COUNTER.get(device)
    if c is None:
        c = (torch.zeros(1, dtype=torch.int32, device=device), torch.zeros(1, dtype=torch.int32).pin_memory())
        _BAND_COUNTER[device] = c
        _BAND_STATE.update(pending=None, launched=0, seen=(0, 0))
    return c


def _band_policy_allows():
    st = _BAND_STATE
    pend = st['pending']
    if pend is not None and pend[1].query():
        redone_total, launched_total = int(pend[0].item()), pend[2]
        redone, batch = redone_total - st['seen'][0], launched_total - st['seen'][1]
        st['seen'] = (redone_total, launched_total)
        st['pending'] = None
        if redone * 10 > batch:
            st['cool'] = _BAND_COOLDOWN
    if st['cool'] > 0:
        st['cool'] -= 1
        return False
    return True


def _band_policy_record(device, B):
    """the kernel's running redo counter, read without a sync (pinned copy + event) once in a while"""
    st = _BAND_STATE
    st['launched'] += B
    if st['pending'] is not None:
        return
    dev_cnt, host = _band_counter(device)
    host.copy_(dev_cnt, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    st['pending'] = (host, ev, st['launched'])


def scale_rows_(x, scale):
    """asr_scale_rows_f32: x [T,B,C] *= scale [B] in place; utterances whose factor is exactly 1
    are not touched."""
    x = _dev(x, torch.float32, 'x')
    scale = _dev(scale.to(torch.float32), torch.float32, 'scale')
    T, B, C = x.shape
    check(lib().asr_scale_rows_f32(_p(x), T, B, C, _p(scale), _stream()), 'asr_scale_rows_f32')
    return x


def lattice_fwbw(lp, lens, graph, neg_inf=-1e20, want_bwd_total=False, grad_sign=1.0):
    """asr_lattice_fwbw_f32: returns (logZ [B], grad [T,B,C], logZ_bwd|None); grad_sign = -1:
    the occupancies come back negated (asr_lattice_fwbw_signed_f32: the gradient of -logZ)."""
    lp = _dev(lp, torch.float32, 'log_probs')
    lens = _dev(lens, torch.int32, 'act_lens')
    T, B, C = lp.shape
    if graph.Bg not in (1, B):
        raise AssertionError("graph batch %d not in (1, %d)" % (graph.Bg, B))
    L = lib()
    logZ = torch.empty(B, dtype=torch.float32, device=lp.device)
    grad = torch.empty_like(lp)
    zb = torch.empty(B, dtype=torch.float32, device=lp.device) if want_bwd_total else None
    if (T + 64) * B * C * 4 >= 2 ** 32 and graph.N <= 512 and not _WARNED.get('fits32'):
        _WARNED['fits32'] = True        # csrc/lattice.hip: 32-bit buffer offsets in the fast kernels
        warnings.warn('lattice_fwbw: T*B*C*4 = %.2f GiB >= 4 GiB (e.g. bi-char CTC at B >= ~1100): the '
                      'meet-in-the-middle kernels address with 32-bit offsets, this call runs the '
                      'generic (much slower) kernel; split the batch' % (T * B * C * 4 / 2.0 ** 30))
    nbytes = L.asr_lattice_fwbw_workspace_bytes(T, B, C, graph.N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=lp.device)
    hook = EVENT_HOOK
    if hook is not None:
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record()
    # band lattices (CTC chains of mono-character transcripts): the linear-domain kernel
    # (csrc/lattice_band.inc).  ASR_LATTICE_BAND: 0 never (the log-domain
    # state-labelled kernel, for A/B runs), 2 always, 1 (default) unless most of a recent batch
    # had to be redone in the log domain
    band_env = os.environ.get('ASR_LATTICE_BAND', '1')
    use_band = (graph.band and band_env != '0' and
                L.asr_lattice_fwbw_band_supported(T, B, C, graph.N, graph.Kin, graph.Kout, graph.Bg))
    if use_band and band_env != '2' and (B > _BAND_MAX_BATCH or not _band_policy_allows()):
        use_band = False
    args = (_p(lp), T, B, C, _p(lens), _p(graph.src_in), _p(graph.il_in),
            _p(graph.w_in), _p(graph.term), _p(graph.dst_out), _p(graph.il_out),
            _p(graph.w_out), graph.N, graph.Kin, graph.Kout, graph.Bg,
            float(neg_inf), _p(logZ), _p(grad), _p(zb), _p(ws), nbytes)
    sargs = args[:17] + (float(grad_sign),) + args[17:]
    if use_band:
        cl = getattr(graph, 'ctc_labels', None)
        if cl is not None and os.environ.get('ASR_BAND_LABELS', '1') == '0':
            cl = None
        check(L.asr_lattice_fwbw_band_f32(*sargs, _p(_band_counter(lp.device)[0]),
                                          _p(cl[0]) if cl else None, _p(cl[1]) if cl else None,
                                          int(cl[0].shape[1]) if cl else 0, _stream()),
              'asr_lattice_fwbw_band_f32')
    elif grad_sign != 1.0:
        check(L.asr_lattice_fwbw_signed_f32(*sargs, _stream()), 'asr_lattice_fwbw_signed_f32')
    else:
        check(L.asr_lattice_fwbw_f32(*args, _stream()), 'asr_lattice_fwbw_f32')
    if hook is not None:
        ev1.record()
        hook.append((ev0, ev1))
    if use_band and band_env != '2':
        _band_policy_record(lp.device, B)
    if graph.addend is not None:
        logZ += graph.addend
        if zb is not None:
            zb += graph.addend
    if use_band and os.environ.get('ASR_LATTICE_BAND_DEBUG'):
        # development aid: why utterances were redone by the in-kernel log-domain body (the last
        # word of each utterance's workspace region, csrc/lattice_band.inc); synchronises
        wc = (graph.N + 63) // 64 * 64 + 64
        why = ws[:B * (T + 2) * wc * 4].view(torch.int32).view(B, (T + 2) * wc)[:, -1].cpu()
        vals, cnts = torch.unique(why, return_counts=True)
        print('[band] B=%d T=%d N=%d fallback reasons {code: utterances} %s' % (
            B, T, graph.N, dict(zip(vals.tolist(), cnts.tolist()))), flush=True)
    return logZ, grad, zb


def lattice_forward(lp, lens, graph, neg_inf=-1e20, viterbi=False, want_path=False):
    """asr_lattice_forward_f32: returns (score [B], best_il [T,B] | None)."""
    lp = _dev(lp, torch.float32, 'log_probs')
    lens = _dev(lens, torch.int32, 'act_lens')
    T, B, C = lp.shape
    if graph.Bg not in (1, B):
        raise AssertionError("graph batch %d not in (1, %d)" % (graph.Bg, B))
    L = lib()
    score = torch.empty(B, dtype=torch.float32, device=lp.device)
    best, ws, nbytes = None, None, 0
    if viterbi and want_path:
        best = torch.empty((T, B), dtype=torch.int32, device=lp.device)
        nbytes = L.asr_lattice_viterbi_workspace_bytes(T, B, graph.N)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=lp.device)
    check(L.asr_lattice_forward_f32(
        _p(lp), T, B, C, _p(lens), _p(graph.src_in), _p(graph.il_in),
        _p(graph.w_in), _p(graph.term), graph.N, graph.Kin, graph.Bg,
        float(neg_inf), int(bool(viterbi)), _p(score), _p(best), _p(ws), nbytes,
        _stream()), 'asr_lattice_forward_f32')
    if graph.addend is not None:
        score += graph.addend
    return score, best


def log_softmax_fwd(x, group):
    x = _dev(x, torch.float32, 'acts')
    if x.numel() % group:
        raise AssertionError("group %d does not divide %d" % (group, x.numel()))
    y = torch.empty_like(x)
    check(lib().asr_log_softmax_fwd_f32(_p(x), x.numel() // group, group, _p(y),
                                        _stream()), 'asr_log_softmax_fwd_f32')
    return y


def log_softmax_bwd(y, dy, group):
    y = _dev(y, torch.float32, 'y')
    dy = _dev(dy, torch.float32, 'dy')
    dx = torch.empty_like(y)
    check(lib().asr_log_softmax_bwd_f32(_p(y), _p(dy), y.numel() // group, group,
                                        _p(dx), _stream()),
          'asr_log_softmax_bwd_f32')
    return dx


def sub_rowmax(x, lens):
    """asr_sub_rowmax_f32: returns (x - rowmax, row_max [T,B], max_sum [B])."""
    x = _dev(x, torch.float32, 'logits')
    lens = _dev(lens, torch.int32, 'lens')
    T, B, C = x.shape
    y = torch.empty_like(x)
    row_max = torch.empty((T, B), dtype=torch.float32, device=x.device)
    max_sum = torch.empty(B, dtype=torch.float32, device=x.device)
    check(lib().asr_sub_rowmax_f32(_p(x), T, B, C, _p(lens), _p(y), _p(row_max),
                                   _p(max_sum), _stream()), 'asr_sub_rowmax_f32')
    return y, row_max, max_sum


def argmax_rows(x):
    """asr_argmax_rows_f32 over the last axis: returns int32 indices x.shape[:-1]."""
    x = _dev(x, torch.float32, 'logits')
    C = x.shape[-1]
    out = torch.empty(x.shape[:-1], dtype=torch.int32, device=x.device)
    check(lib().asr_argmax_rows_f32(_p(x), x.numel() // C, C, _p(out), _stream()),
          'asr_argmax_rows_f32')
    return out


_LSTM_ERR = {}      # device index -> int32[1] timeout word of the persistent recurrence


def _lstm_err_flag(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    f = _LSTM_ERR.get(idx)
    if f is None:
        f = _LSTM_ERR[idx] = torch.zeros(1, dtype=torch.int32, device=device)
    return f


def lstm_error_word(device):
    """The device word a timed-out hand-off of the persistent recurrence sets (int32[1]), or None
    when no recurrence has run on `device`; `dp.train_step` folds it into its one read-back."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return _LSTM_ERR.get(idx)


def lstm_raise_error(word):
    word.zero_()
    raise RuntimeError(
        'persistent BiLSTM / BiGRU recurrence: a team hand-off timed out (another stream\'s kernel kept a '
        'team mate off the device?); the outputs of that call, and the gradients of this step on '
        'every rank, are NaN: the step is discarded. Set ASR_LSTM_PERSIST=0 to use one launch per '
        'time step.')


def lstm_check_errors():
    """Raise if a hand-off of the persistent BiLSTM / BiGRU recurrence timed out since the last
    check (csrc/lstm.hip team_wait: the kernel then poisons its outputs with NaN; the
    step must be discarded).  One 4-byte read-back per device; `dp.train_step` calls it
    once per step."""
    for idx, f in _LSTM_ERR.items():
        if int(f.item()) != 0:
            f.zero_()
            raise RuntimeError(
                'persistent BiLSTM / BiGRU recurrence: a team hand-off timed out on cuda:%d (another '
                "stream's kernel kept a team mate off the device?); outputs of that call are "
                'NaN. Set ASR_LSTM_PERSIST=0 to use one launch per time step.' % idx)


def lstm_bidir_fwd(gx, whh_bf16, lens, want_y=True):
    """asr_lstm_bidir_fwd_bf16: gx [T,B,2,4H] f32 or bf16, whh [2,4H,H] bf16, lens [B] i32
    -> (y [T,B,2,H] f32, y_bf16 [2,T+2,B,H], gates [T,2,B,H,4] bf16, csave [T,2,B,H])."""
    gx = _dev(gx, gx.dtype if gx.dtype == torch.bfloat16 else torch.float32, 'gx')
    whh_bf16 = _dev(whh_bf16, torch.bfloat16, 'whh')
    lens = _dev(lens, torch.int32, 'lens')
    T, B, _, H4 = gx.shape
    H = H4 // 4
    L = lib()
    y = torch.empty((T, B, 2, H), dtype=torch.float32, device=gx.device) if want_y else None
    ybf = torch.empty((2, T + 2, B, H), dtype=torch.bfloat16, device=gx.device)
    gates = torch.empty((T, 2, B, H, 4), dtype=torch.bfloat16, device=gx.device)
    csave = torch.empty((T, 2, B, H), dtype=torch.float32, device=gx.device)
    nbytes = L.asr_lstm_workspace_bytes(B, H)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gx.device)
    check(L.asr_lstm_bidir_fwd_bf16(_p(gx), int(gx.dtype == torch.bfloat16), _p(whh_bf16),
                                    _p(lens), T, B, H, _p(y),
                                    _p(ybf), _p(gates), _p(csave), _p(ws), nbytes,
                                    _p(_lstm_err_flag(gx.device)), _stream()), 'asr_lstm_bidir_fwd_bf16')
    return y, ybf, gates, csave


def lstm_fused_supported(B, H, F=None):
    """asr_lstm_fused_supported: can asr_lstm_bidir_fwd_fused_bf16 run this (batch, hidden,
    input size)?"""
    F = H if F is None else F
    return bool(lib().asr_lstm_fused_supported(int(B), int(H), int(F)) & 1)


def lstm_bidir_fwd_fused(x_bf16, wih_bf16, whh_bf16, lens, want_y=True):
    """asr_lstm_bidir_fwd_fused_bf16: x [T,B,F] bf16, wih [2*4H,F] bf16, whh [2,4H,H] bf16
    -> the outputs of lstm_bidir_fwd, the input projection computed inside the recurrence."""
    x_bf16 = _dev(x_bf16, torch.bfloat16, 'x')
    wih_bf16 = _dev(wih_bf16, torch.bfloat16, 'wih')
    whh_bf16 = _dev(whh_bf16, torch.bfloat16, 'whh')
    lens = _dev(lens, torch.int32, 'lens')
    T, B, F = x_bf16.shape
    H = whh_bf16.shape[-1]
    if tuple(wih_bf16.shape) != (8 * H, F) or tuple(whh_bf16.shape) != (2, 4 * H, H):
        raise ValueError('lstm_bidir_fwd_fused: wih must be [8H, F], whh [2, 4H, H]')
    L = lib()
    dev = x_bf16.device
    y = torch.empty((T, B, 2, H), dtype=torch.float32, device=dev) if want_y else None
    ybf = torch.empty((2, T + 2, B, H), dtype=torch.bfloat16, device=dev)
    gates = torch.empty((T, 2, B, H, 4), dtype=torch.bfloat16, device=dev)
    csave = torch.empty((T, 2, B, H), dtype=torch.float32, device=dev)
    nbytes = L.asr_lstm_workspace_bytes(B, H)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.asr_lstm_bidir_fwd_fused_bf16(_p(x_bf16), _p(wih_bf16), _p(whh_bf16), _p(lens), T, B, H, F,
                                          _p(y), _p(ybf), _p(gates), _p(csave), _p(ws), nbytes,
                                          _p(_lstm_err_flag(dev)), _stream()),
          'asr_lstm_bidir_fwd_fused_bf16')
    return y, ybf, gates, csave


def lens_on(lens, device):
    """int32 device copy of a CPU length vector.  A host-to-device copy in the middle of a
    step waits for everything queued before it (pageable memory), after which the small
    kernels that follow run at the host's launch rate; whoever creates the lengths early in
    the step (DeepSpeech2.forward) can attach the device copy with `attach_device_lens` and
    every later consumer picks it up here."""
    if not isinstance(lens, torch.Tensor):
        lens = torch.as_tensor(lens)
    if lens.is_cuda:
        return lens.to(device=device, dtype=torch.int32)
    hit = getattr(lens, '_asr_dev', None)
    if hit is not None and hit[0] == str(device) and hit[1] == lens._version:
        return hit[2]
    return lens.to(device=device, dtype=torch.int32)


def attach_device_lens(lens, device):
    """copy a CPU length vector to the device now and remember the copy on the tensor object"""
    if isinstance(lens, torch.Tensor) and not lens.is_cuda:
        lens._asr_dev = (str(device), lens._version, lens.to(device=device, dtype=torch.int32))
    return lens


def lstm_dgrad_supported(H):
    return bool(lib().asr_lstm_dgrad_supported(int(H)))


def lstm_dgrad(dgates, w_ih_bf16):
    """asr_lstm_dgrad_bf16: dgates [T,B,2,4H] bf16, w_ih [8H,H] bf16 -> dx [T,B,H] f32."""
    dgates = _dev(dgates, torch.bfloat16, 'dgates')
    w_ih_bf16 = _dev(w_ih_bf16, torch.bfloat16, 'w_ih')
    T, B, H = dgates.shape[0], dgates.shape[1], dgates.shape[3] // 4
    if tuple(w_ih_bf16.shape) != (8 * H, H):
        raise ValueError('lstm_dgrad: w_ih must be [8H, H]')
    dx = torch.empty((T, B, H), dtype=torch.float32, device=dgates.device)
    check(lib().asr_lstm_dgrad_bf16(_p(dgates), _p(w_ih_bf16), T, B, H, _p(dx), _stream()),
          'asr_lstm_dgrad_bf16')
    return dx


def lstm_wgrad_supported(H):
    return bool(lib().asr_lstm_wgrad_supported(int(H)))


def lstm_wgrad(dgates, x_bf16, y_bf16):
    """asr_lstm_wgrad_bf16: dgates [T,B,2,4H] bf16, x [T*B,H] bf16 or None, y_bf16 [2,T+2,B,H]
    -> (dw_ih [8H,H] f32 or None, dw_hh [2,4H,H] f32)."""
    dgates = _dev(dgates, torch.bfloat16, 'dgates')
    y_bf16 = _dev(y_bf16, torch.bfloat16, 'y_bf16')
    T, B, H = dgates.shape[0], dgates.shape[1], dgates.shape[3] // 4
    dev = dgates.device
    if x_bf16 is not None:
        x_bf16 = _dev(x_bf16, torch.bfloat16, 'x')
        if x_bf16.numel() != T * B * H:
            raise ValueError('lstm_wgrad: x must be [T*B, H]')
    L = lib()
    dw_ih = torch.empty((8 * H, H), dtype=torch.float32, device=dev) if x_bf16 is not None else None
    dw_hh = torch.empty((2, 4 * H, H), dtype=torch.float32, device=dev)
    nbytes = L.asr_lstm_wgrad_workspace_bytes(T, B, H, int(x_bf16 is not None))
    if nbytes < 0:
        raise NativeLibraryError('asr_lstm_wgrad: unsupported hidden size %d' % H)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.asr_lstm_wgrad_bf16(_p(dgates), _p(x_bf16), _p(y_bf16), T, B, H, _p(dw_ih), _p(dw_hh),
                                _p(ws), nbytes, _stream()), 'asr_lstm_wgrad_bf16')
    return dw_ih, dw_hh


def lstm_bidir_bwd(dy, whhT_bf16, lens, gates, csave):
    """asr_lstm_bidir_bwd_bf16 -> dgates [T,B,2,4H] bf16.  dy [T,B,2,H], or [T,B,H] when
    the two directions share one gradient (their outputs are summed)."""
    dy = _dev(dy, torch.float32, 'dy')
    whhT_bf16 = _dev(whhT_bf16, torch.bfloat16, 'whhT')
    lens = _dev(lens, torch.int32, 'lens')
    T, B, H = dy.shape[0], dy.shape[1], dy.shape[-1]
    L = lib()
    dgates = torch.empty((T, B, 2, 4 * H), dtype=torch.bfloat16, device=dy.device)
    nbytes = L.asr_lstm_workspace_bytes(B, H)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dy.device)
    check(L.asr_lstm_bidir_bwd_bf16(_p(dy), int(dy.dim() == 3), _p(whhT_bf16), _p(lens), T, B, H,
                                    _p(gates), _p(csave), _p(dgates), _p(ws), nbytes,
                                    _p(_lstm_err_flag(dy.device)), _stream()),
          'asr_lstm_bidir_bwd_bf16')
    return dgates


def gru_supported(B, H):
    """asr_gru_supported: is the GRU recurrence built for this (batch, hidden size)?"""
    return bool(lib().asr_gru_supported(int(B), int(H)) & 1)


def gru_bidir_fwd(gx, whh_bf16, lens):
    """asr_gru_bidir_fwd_bf16: gx [T,B,2,3H] f32 or bf16, whh [2,3H,H] bf16, lens [B] i32
    -> (y [T,B,2,H] f32, y_bf16 [2,T+2,B,H], gates [T,2,B,H,4] bf16 records (r, z, n, hn)).
    Shares the LSTM's error word (lstm_check_errors)."""
    gx = _dev(gx, gx.dtype if gx.dtype == torch.bfloat16 else torch.float32, 'gx')
    whh_bf16 = _dev(whh_bf16, torch.bfloat16, 'whh')
    lens = _dev(lens, torch.int32, 'lens')
    T, B, _, H3 = gx.shape
    H = H3 // 3
    if tuple(whh_bf16.shape) != (2, 3 * H, H):
        raise ValueError('gru_bidir_fwd: whh must be [2, 3H, H]')
    L = lib()
    dev = gx.device
    y = torch.empty((T, B, 2, H), dtype=torch.float32, device=dev)
    ybf = torch.empty((2, T + 2, B, H), dtype=torch.bfloat16, device=dev)
    gates = torch.empty((T, 2, B, H, 4), dtype=torch.bfloat16, device=dev)
    nbytes = L.asr_gru_workspace_bytes(B, H)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.asr_gru_bidir_fwd_bf16(_p(gx), int(gx.dtype == torch.bfloat16), _p(whh_bf16), _p(lens),
                                   T, B, H, _p(y), _p(ybf), _p(gates), _p(ws), nbytes,
                                   _p(_lstm_err_flag(dev)), _stream()), 'asr_gru_bidir_fwd_bf16')
    return y, ybf, gates


def gru_bidir_bwd(dy, whhT_bf16, lens, gates, y):
    """asr_gru_bidir_bwd_bf16 -> (dgx [T,B,2,3H] bf16 = (dr, dz, dn), dhn [T,B,2,H] bf16).
    dy [T,B,2,H], or [T,B,H] when the two directions share one gradient; whhT [2,H,3H] bf16;
    gates, y: what gru_bidir_fwd returned."""
    dy = _dev(dy, torch.float32, 'dy')
    whhT_bf16 = _dev(whhT_bf16, torch.bfloat16, 'whhT')
    lens = _dev(lens, torch.int32, 'lens')
    gates = _dev(gates, torch.bfloat16, 'gates')
    y = _dev(y, torch.float32, 'y')
    T, B, H = dy.shape[0], dy.shape[1], dy.shape[-1]
    if tuple(whhT_bf16.shape) != (2, H, 3 * H) or tuple(y.shape) != (T, B, 2, H):
        raise ValueError('gru_bidir_bwd: whhT must be [2, H, 3H], y [T, B, 2, H]')
    L = lib()
    dev = dy.device
    dgx = torch.empty((T, B, 2, 3 * H), dtype=torch.bfloat16, device=dev)
    dhn = torch.empty((T, B, 2, H), dtype=torch.bfloat16, device=dev)
    nbytes = L.asr_gru_workspace_bytes(B, H)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.asr_gru_bidir_bwd_bf16(_p(dy), int(dy.dim() == 3), _p(whhT_bf16), _p(lens), T, B, H,
                                   _p(gates), _p(y), _p(dgx), _p(dhn), _p(ws), nbytes,
                                   _p(_lstm_err_flag(dev)), _stream()), 'asr_gru_bidir_bwd_bf16')
    return dgx, dhn


class GroupedGraph(object):
    """Device copy of a group-factored decoding graph (include/asr_amd.h,
    asr_lattice_grouped_*): numpy/torch arrays g_of, h_of, label, selfx, uniq [N],
    mem_g [G,Wg], mem_h [G,Wh], term [N]."""

    def __init__(self, st, device):
        def i32(a):
            return torch.as_tensor(a).to(device=device, dtype=torch.int32).contiguous()
        self.g_of, self.h_of, self.label = i32(st['g_of']), i32(st['h_of']), i32(st['label'])
        self.selfx, self.uniq = i32(st['selfx']), i32(st['uniq'])
        self.mem_g, self.mem_h = i32(st['mem_g']), i32(st['mem_h'])
        self.term = torch.as_tensor(st['term']).to(device=device, dtype=torch.float32).contiguous()
        self.N = int(self.g_of.numel())
        self.G, self.Wg = self.mem_g.shape
        self.Wh = self.mem_h.shape[1]

    def _args(self):
        return (self.N, self.G, self.Wg, self.Wh, _p(self.g_of), _p(self.h_of), _p(self.label),
                _p(self.selfx), _p(self.uniq), _p(self.mem_g), _p(self.mem_h), _p(self.term))


def grouped_fwbw(lp, lens, gg, neg_inf=-1e20, want_bwd_total=False, add_to=None):
    """asr_lattice_grouped_fwbw_f32 -> (logZ [B], grad [T,B,C], logZ_bwd | None); add_to: a
    [T,B,C] f32 tensor the occupancies are ADDED to (asr_lattice_grouped_fwbw_acc_f32) and which
    is returned as grad."""
    lp = _dev(lp, torch.float32, 'log_probs')
    lens = _dev(lens, torch.int32, 'act_lens')
    T, B, C = lp.shape
    L = lib()
    logZ = torch.empty(B, dtype=torch.float32, device=lp.device)
    if add_to is not None:
        assert add_to.shape == lp.shape and add_to.is_contiguous() and add_to.dtype == torch.float32
    grad = torch.empty_like(lp) if add_to is None else add_to
    zb = torch.empty(B, dtype=torch.float32, device=lp.device) if want_bwd_total else None
    nbytes = L.asr_lattice_grouped_workspace_bytes(T, B, gg.N, gg.G)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=lp.device)
    check(L.asr_lattice_grouped_fwbw_acc_f32(
        _p(lp), T, B, C, _p(lens), *gg._args(), float(neg_inf), int(add_to is not None), _p(logZ),
        _p(grad), _p(zb), _p(ws), nbytes, _stream()), 'asr_lattice_grouped_fwbw_acc_f32')
    return logZ, grad, zb


def grouped_forward(lp, lens, gg, neg_inf=-1e20, viterbi=False, want_path=False):
    """asr_lattice_grouped_forward_f32 -> (score [B], best_il [T,B] | None)."""
    lp = _dev(lp, torch.float32, 'log_probs')
    lens = _dev(lens, torch.int32, 'act_lens')
    T, B, C = lp.shape
    L = lib()
    score = torch.empty(B, dtype=torch.float32, device=lp.device)
    best, ws, nbytes = None, None, 0
    if viterbi and want_path:
        best = torch.empty((T, B), dtype=torch.int32, device=lp.device)
        nbytes = L.asr_lattice_grouped_workspace_bytes(T, B, gg.N, gg.G)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=lp.device)
    check(L.asr_lattice_grouped_forward_f32(
        _p(lp), T, B, C, _p(lens), *gg._args(), float(neg_inf), int(bool(viterbi)), _p(score),
        _p(best), _p(ws), nbytes, _stream()), 'asr_lattice_grouped_forward_f32')
    return score, best


class SharedGraph(object):
    """Device copy of a shared weighted sparse graph in CSR form (include/asr_amd.h,
    asr_lattice_shared_*), from the bundle fst_utils.shared_structure makes: in_ptr / out_ptr
    [N+1], in_nb / in_il / in_w and out_nb / out_il / out_w [E] (neighbour state, input label,
    weight), term [N].  The degree-ordered state lists and the lanes per state are worked out
    here."""
    HEAVY = 128          # arcs from which a state gets a whole wave

    def __init__(self, st, device):
        import numpy as np
        self.N, self.E = int(len(st['term'])), int(len(st['in_w']))
        self.C_min = int(max(st['in_il'].max(), 0)) + 1 if self.E else 1
        if self.N > 65535 or self.C_min > 65536:
            raise NotImplementedError('shared graph: 16-bit state / label indices')

        def i32(a):
            return torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=torch.int32).contiguous()

        def arcs(nb, il, w):
            rec = np.empty((self.E, 2), np.uint32)
            rec[:, 0] = np.asarray(nb, np.uint32) | (np.asarray(il, np.uint32) << np.uint32(16))
            rec[:, 1] = np.asarray(w, np.float32).view(np.uint32)
            return torch.from_numpy(rec.view(np.int32)).to(device).contiguous()

        def order(ptr):
            deg = np.diff(np.asarray(ptr, np.int64))
            idx = np.argsort(-deg, kind='stable')            # equal work side by side in a wave
            heavy = deg[idx] > self.HEAVY
            idx = np.concatenate([idx[~heavy], idx[heavy]])
            n_light = int((~heavy).sum())
            mean = float(deg[deg <= self.HEAVY].mean()) if n_light else 1.0
            lanes = 1
            while lanes < 64 and lanes * 2 * n_light <= 1024 and lanes * 2 <= max(1.0, mean):
                lanes *= 2
            return i32(idx), n_light, lanes, int(deg.max()) if len(deg) else 0
        self.in_ptr, self.out_ptr = i32(st['in_ptr']), i32(st['out_ptr'])
        self.in_arc = arcs(st['in_nb'], st['in_il'], st['in_w'])
        self.out_arc = arcs(st['out_nb'], st['out_il'], st['out_w'])
        self.term = torch.as_tensor(np.asarray(st['term'], np.float32)).to(device).contiguous()
        self.order_in, self.n_light_in, self.lanes_in, self.max_in = order(st['in_ptr'])
        self.order_out, self.n_light_out, self.lanes_out, _ = order(st['out_ptr'])

    def supported(self, C):
        return bool(self.E > 0 and self.max_in <= 65535 and C >= self.C_min and
                    lib().asr_lattice_shared_supported(self.N, self.E, int(C)))


def shared_fwbw(lp, lens, sg, neg_inf=-1e20, want_bwd_total=False, add_to=None, grad_sign=1.0):
    """asr_lattice_shared_fwbw_f32 -> (logZ [B], grad [T,B,C], logZ_bwd | None); add_to: a
    [T,B,C] f32 tensor the occupancies (times grad_sign) are ADDED to and which is returned as
    grad."""
    lp = _dev(lp, torch.float32, 'log_probs')
    lens = _dev(lens, torch.int32, 'act_lens')
    T, B, C = lp.shape
    if C < sg.C_min:
        raise AssertionError('graph consumes label %d, log_probs have %d classes' % (sg.C_min - 1, C))
    L = lib()
    logZ = torch.empty(B, dtype=torch.float32, device=lp.device)
    if add_to is not None:
        assert add_to.shape == lp.shape and add_to.is_contiguous() and add_to.dtype == torch.float32
    grad = torch.empty_like(lp) if add_to is None else add_to
    zb = torch.empty(B, dtype=torch.float32, device=lp.device) if want_bwd_total else None
    nbytes = L.asr_lattice_shared_workspace_bytes(T, B, sg.N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=lp.device)
    check(L.asr_lattice_shared_fwbw_f32(
        _p(lp), T, B, C, _p(lens), sg.N, sg.E, _p(sg.in_ptr), _p(sg.in_arc), _p(sg.out_ptr),
        _p(sg.out_arc), _p(sg.term), _p(sg.order_in), sg.n_light_in, sg.lanes_in, _p(sg.order_out),
        sg.n_light_out, sg.lanes_out, float(neg_inf), float(grad_sign), int(add_to is not None),
        _p(logZ), _p(grad), _p(zb), _p(ws), nbytes, _stream()), 'asr_lattice_shared_fwbw_f32')
    return logZ, grad, zb


def shared_forward(lp, lens, sg, neg_inf=-1e20, viterbi=False, want_path=False):
    """asr_lattice_shared_forward_f32 -> (score [B], best_il [T,B] | None)."""
    lp = _dev(lp, torch.float32, 'log_probs')
    lens = _dev(lens, torch.int32, 'act_lens')
    T, B, C = lp.shape
    if C < sg.C_min:
        raise AssertionError('graph consumes label %d, log_probs have %d classes' % (sg.C_min - 1, C))
    L = lib()
    score = torch.empty(B, dtype=torch.float32, device=lp.device)
    best, ws, nbytes = None, None, 0
    if viterbi and want_path:
        best = torch.empty((T, B), dtype=torch.int32, device=lp.device)
        nbytes = L.asr_lattice_shared_workspace_bytes(T, B, sg.N)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=lp.device)
    check(L.asr_lattice_shared_forward_f32(
        _p(lp), T, B, C, _p(lens), sg.N, sg.E, _p(sg.in_ptr), _p(sg.in_arc), _p(sg.term),
        _p(sg.order_in), sg.n_light_in, sg.lanes_in, float(neg_inf), int(bool(viterbi)), _p(score),
        _p(best), _p(ws), nbytes, _stream()), 'asr_lattice_shared_forward_f32')
    return score, best


def build_ctc_graph(labels, label_lens, num_symbols, context_order,
                    allow_nonblank_selfloops=True, use_contextual_blanks=False,
                    nc_weight=-1e20):
    """asr_ctc_graph_build: labels [B,Lmax] i32 (GPU), label_lens [B] i32 (GPU)
    -> Graph with [B, 2*Lmax+1, 3] arc arrays built on the device."""
    labels = _dev(labels, torch.int32, 'labels')
    label_lens = _dev(label_lens, torch.int32, 'label_lens')
    B, Lmax = labels.shape
    N = 2 * Lmax + 1
    dev = labels.device
    g = Graph(None, dev)

    def ti():
        return torch.empty((B, N, 3), dtype=torch.int32, device=dev)

    def tf():
        return torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    g.src_in, g.il_in, g.w_in = ti(), ti(), tf()
    g.dst_out, g.il_out, g.w_out = ti(), ti(), tf()
    g.term = torch.empty((B, N), dtype=torch.float32, device=dev)
    g.Bg, g.N, g.Kin, g.Kout = B, N, 3, 3
    g.band = True        # the 2 L + 1 chain in natural state order, both context orders
    # mono-character chains: the band kernel writes the chain down from the transcript itself
    g.ctc_labels = (labels, label_lens) if int(context_order) == 1 and Lmax > 0 else None
    check(lib().asr_ctc_graph_build(
        _p(labels), _p(label_lens), B, Lmax, int(num_symbols), int(context_order),
        int(bool(allow_nonblank_selfloops)), int(bool(use_contextual_blanks)),
        float(nc_weight), _p(g.src_in), _p(g.il_in), _p(g.w_in), _p(g.term),
        _p(g.dst_out), _p(g.il_out), _p(g.w_out), _stream()), 'asr_ctc_graph_build')
    return g


def _nchw_or_nhwc(t, name, dtype):
    """4-D GPU tensor as stored: (tensor, channels_last flag) without a layout copy when it
    is dense in either format."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NativeLibraryError(
            "%s must be a GPU tensor: the MI355X path has no CPU fallback" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if t.is_contiguous():
        return t, False
    if t.is_contiguous(memory_format=torch.channels_last):
        return t, True
    return t.contiguous(), False


def bn_act_fwd(x, gamma, beta, running_mean, running_var, training, momentum, eps, lo, hi,
               out_bf16=False, time_major=False, conv_bias=None, chan_sums=None):
    """asr_bn_act_fwd_f32 on x [B,C,H,W] f32 (NCHW or channels_last storage) or bf16
    (channels_last) ->
    (out, save_mean [C], save_invstd [C]); out is [B,C,H,W] in x's memory format or,
    time_major, a dense [H,B,C,W]; running stats are updated in place when training."""
    x, cl = _nchw_or_nhwc(x, 'x', x.dtype if x.dtype == torch.bfloat16 else torch.float32)
    gamma = _dev(gamma, torch.float32, 'gamma')
    beta = _dev(beta, torch.float32, 'beta')
    B, C, H, W = x.shape
    if cl and (C % 4 or C > 1024 or 256 % (C // 4)):
        x, cl = x.contiguous(), False
    if x.dtype == torch.bfloat16 and not cl:        # bf16 input is a channels-last path
        x = x.float()
    L = lib()
    odt = torch.bfloat16 if out_bf16 else torch.float32
    if time_major:
        out = torch.empty((H, B, C, W), dtype=odt, device=x.device)
    else:
        out = torch.empty((B, C, H, W), dtype=odt, device=x.device,
                          memory_format=torch.channels_last if cl else torch.contiguous_format)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    nbytes = L.asr_bn_act_workspace_bytes(C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    if conv_bias is not None:
        conv_bias = _dev(conv_bias, torch.float32, 'conv_bias')
    check(L.asr_bn_act_fwd_f32(_p(x), int(x.dtype == torch.bfloat16), _p(conv_bias), B, C, H, W, _p(gamma), _p(beta), _p(running_mean),
                               _p(running_var), int(cl), int(bool(training)), float(momentum),
                               float(eps), float(lo), float(hi), _p(out), int(out_bf16),
                               int(time_major), _p(mean), _p(invstd), _p(chan_sums), _p(ws), nbytes,
                               _stream()),
          'asr_bn_act_fwd_f32')
    return out, mean, invstd


def bn_act_bwd(x, gamma, beta, mean, invstd, training, lo, hi, dy, time_major=False,
               conv_bias=None, sync=None):
    """asr_bn_act_bwd_f32 -> (dx [B,C,H,W] f32 in x's memory format, dgamma [C], dbeta [C],
    dconv_bias [C] | None);
    dy f32 or bf16 in the layout the forward wrote.
    sync: a callable (sums [2 C] f64 device tensor, n_local) -> n_total that adds the per-channel
    sums up over the replicas in place (SyncBN-style data parallelism): the call then runs as
    asr_bn_act_bwd_phase_f32 phase 1 (local sums + parameter gradients), sync, phase 2 (dx)."""
    x, cl = _nchw_or_nhwc(x, 'x', x.dtype if x.dtype == torch.bfloat16 else torch.float32)
    if cl and (x.shape[1] % 4 or x.shape[1] > 1024 or 256 % (x.shape[1] // 4)):
        x, cl = x.contiguous(), False
    if x.dtype == torch.bfloat16 and not cl:
        x = x.float()
    if dy.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("dy must be float32 or bfloat16")
    if time_major or not cl:
        dy = _dev(dy, dy.dtype, 'dy')
    else:
        dy = dy.contiguous(memory_format=torch.channels_last)
    B, C, H, W = x.shape
    L = lib()
    dx = torch.empty_like(x)                      # preserves the memory format
    dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
    dcb = None
    if conv_bias is not None:
        conv_bias = _dev(conv_bias, torch.float32, 'conv_bias')
        dcb = torch.empty(C, dtype=torch.float32, device=x.device)
    nbytes = L.asr_bn_act_workspace_bytes(C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    if sync is not None and training:
        def phase(k, n_total):
            check(L.asr_bn_act_bwd_phase_f32(
                _p(x), int(x.dtype == torch.bfloat16), _p(conv_bias), B, C, H, W, _p(gamma), _p(beta),
                _p(mean), _p(invstd), int(cl), 1, float(lo), float(hi), _p(dy),
                int(dy.dtype == torch.bfloat16), int(time_major), _p(dx), _p(dgamma), _p(dbeta), _p(dcb),
                _p(ws), nbytes, k, float(n_total), _stream()), 'asr_bn_act_bwd_phase_f32')
        phase(1, 0.0)
        sums = ws[:2 * C * 8].view(torch.float64)
        phase(2, sync(sums, float(B) * H * W))
        return dx, dgamma, dbeta, dcb
    check(L.asr_bn_act_bwd_f32(_p(x), int(x.dtype == torch.bfloat16), _p(conv_bias), B, C, H, W, _p(gamma), _p(beta), _p(mean), _p(invstd),
                               int(cl), int(bool(training)), float(lo), float(hi), _p(dy),
                               int(dy.dtype == torch.bfloat16), int(time_major), _p(dx),
                               _p(dgamma), _p(dbeta), _p(dcb), _p(ws), nbytes, _stream()),
          'asr_bn_act_bwd_f32')
    return dx, dgamma, dbeta, dcb


def bn_act_bwd_sums(x, gamma, beta, mean, invstd, training, lo, hi, dy, conv_bias=None):
    """phase 1 of asr_bn_act_bwd_phase_f32 alone, for a consumer that applies phase 2 itself
    (conv1_wgrad_bn): x, dy [B,C,H,W] channels-last bf16 -> (workspace holding the two
    per-channel sums, as f64 in its first 2 C * 8 bytes; dgamma [C]; dbeta [C]; dconv_bias [C]
    | None).  No dx is allocated."""
    x = _nhwc_bf16(x, 'x')[0]
    dy = _nhwc_bf16(dy, 'dy')[0]
    B, C, H, W = x.shape
    L = lib()
    dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
    dcb = None
    if conv_bias is not None:
        conv_bias = _dev(conv_bias, torch.float32, 'conv_bias')
        dcb = torch.empty(C, dtype=torch.float32, device=x.device)
    nbytes = L.asr_bn_act_workspace_bytes(C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    # (dx must be a pointer; phase 1 stores nothing through it)
    check(L.asr_bn_act_bwd_phase_f32(
        _p(x), 1, _p(conv_bias), B, C, H, W, _p(gamma), _p(beta), _p(mean), _p(invstd), 1,
        int(bool(training)), float(lo), float(hi), _p(dy), 1, 0, _p(ws), _p(dgamma), _p(dbeta),
        _p(dcb), _p(ws), nbytes, 1, 0.0, _stream()), 'asr_bn_act_bwd_phase_f32')
    return ws, dgamma, dbeta, dcb


def tcn_attention_step(eproj, enc, enc_lens, filt, glob, w_score, b_score, temperature,
                       att_prev, parent, beam, window=None):
    """asr_tcn_attention_step_f32 -> (att_new [B*beam, T], context [B*beam, E]); with
    `window` = (lo, hi), LocalAttention's force_forward, asr_tcn_attention_step_win_f32."""
    eproj, enc = _dev(eproj, torch.float32, 'eproj'), _dev(enc, torch.float32, 'enc')
    filt, glob = _dev(filt, torch.float32, 'filt'), _dev(glob, torch.float32, 'glob')
    att_prev = _dev(att_prev, torch.float32, 'att_prev')
    w_score = _dev(w_score, torch.float32, 'w_score')
    enc_lens = _dev(enc_lens, torch.int32, 'enc_lens')
    T, B, A = eproj.shape
    E = enc.shape[2]
    hyps = B * beam
    taps = filt.numel() // (hyps * A)
    att_new = torch.empty((hyps, T), dtype=torch.float32, device=enc.device)
    ctx = torch.empty((hyps, E), dtype=torch.float32, device=enc.device)
    par = None if parent is None else _dev(parent, torch.int32, 'parent')
    if window is not None:
        lo, hi = window
        if int(lo) != lo or int(hi) != hi:
            raise TypeError("window must be a pair of integers")
        check(lib().asr_tcn_attention_step_win_f32(
            _p(eproj), _p(enc), _p(enc_lens), _p(filt), _p(glob), _p(w_score), float(b_score),
            float(temperature), _p(att_prev), _p(par), T, B, beam, A, taps, E, int(lo), int(hi),
            _p(att_new), _p(ctx), _stream()), 'asr_tcn_attention_step_win_f32')
        return att_new, ctx
    check(lib().asr_tcn_attention_step_f32(
        _p(eproj), _p(enc), _p(enc_lens), _p(filt), _p(glob), _p(w_score), float(b_score),
        float(temperature), _p(att_prev), _p(par), T, B, beam, A, taps, E, _p(att_new), _p(ctx),
        _stream()), 'asr_tcn_attention_step_f32')
    return att_new, ctx


def _tcn_scan_shapes(what, T, B, L, A, filt, glob, a0, w_score, enc_lens):
    """filt [L, B, A*Kf], glob [L, B, A], a0 [T, B], w_score [A], enc_lens [B]: the kernels index
    every operand by the shape of eproj and the L of glob alone"""
    if (filt.dim() != 3 or tuple(filt.shape[:2]) != (L, B) or filt.shape[2] % A != 0
            or tuple(glob.shape) != (L, B, A) or tuple(a0.shape) != (T, B) or w_score.numel() != A
            or enc_lens.numel() != B):
        raise AssertionError('%s: inconsistent operand shapes' % what)


def tcn_attention_scan_fwd(eproj, filt, glob, a0, w_score, b_score, enc_lens, temperature):
    """asr_tcn_attention_scan_fwd_f32 -> every alignment of the training scan [L, B, T]."""
    eproj, a0 = _dev(eproj, torch.float32, 'eproj'), _dev(a0, torch.float32, 'a0')
    filt, glob = _dev(filt, torch.float32, 'filt'), _dev(glob, torch.float32, 'glob')
    w_score = _dev(w_score, torch.float32, 'w_score')
    b_score = _dev(b_score, torch.float32, 'b_score')
    enc_lens = _dev(enc_lens, torch.int32, 'enc_lens')
    T, B, A = eproj.shape
    L = glob.shape[0]
    _tcn_scan_shapes('asr_tcn_attention_scan_fwd_f32', T, B, L, A, filt, glob, a0, w_score, enc_lens)
    if b_score.numel() != 1:
        raise AssertionError('asr_tcn_attention_scan_fwd_f32: inconsistent operand shapes')
    att = torch.empty((L, B, T), dtype=torch.float32, device=eproj.device)
    check(lib().asr_tcn_attention_scan_fwd_f32(
        _p(eproj), _p(filt), _p(glob), _p(a0), _p(w_score), _p(b_score), float(temperature),
        _p(enc_lens), T, B, L, A, filt.shape[2] // A, _p(att), _stream()),
        'asr_tcn_attention_scan_fwd_f32')
    return att


def tcn_attention_scan_bwd(eproj, filt, glob, a0, w_score, enc_lens, temperature, att, d_att):
    """asr_tcn_attention_scan_bwd_f32 -> (d_eproj [T, B, A], d_filt [L, B, A*Kf],
    d_glob [L, B, A], d_a0 [T, B], d_wb [B, A+1] per-utterance partials of d w / d b)."""
    eproj, a0 = _dev(eproj, torch.float32, 'eproj'), _dev(a0, torch.float32, 'a0')
    filt, glob = _dev(filt, torch.float32, 'filt'), _dev(glob, torch.float32, 'glob')
    w_score = _dev(w_score, torch.float32, 'w_score')
    enc_lens = _dev(enc_lens, torch.int32, 'enc_lens')
    att, d_att = _dev(att, torch.float32, 'att'), _dev(d_att, torch.float32, 'd_att')
    T, B, A = eproj.shape
    L = glob.shape[0]
    _tcn_scan_shapes('asr_tcn_attention_scan_bwd_f32', T, B, L, A, filt, glob, a0, w_score, enc_lens)
    if att.shape != (L, B, T) or d_att.shape != (L, B, T):
        raise AssertionError('asr_tcn_attention_scan_bwd_f32: inconsistent operand shapes')
    d_eproj = torch.empty_like(eproj)
    d_filt = torch.empty_like(filt)
    d_glob = torch.empty_like(glob)
    d_a0 = torch.empty_like(a0)
    d_wb = torch.empty((B, A + 1), dtype=torch.float32, device=eproj.device)
    check(lib().asr_tcn_attention_scan_bwd_f32(
        _p(eproj), _p(filt), _p(glob), _p(a0), _p(w_score), float(temperature), _p(enc_lens),
        _p(att), _p(d_att), T, B, L, A, filt.shape[2] // A, _p(d_eproj), _p(d_filt), _p(d_glob),
        _p(d_a0), _p(d_wb), _stream()), 'asr_tcn_attention_scan_bwd_f32')
    return d_eproj, d_filt, d_glob, d_a0, d_wb


ATT_GRU_MAX_FRAMES, ATT_GRU_MAX_HIDDEN, ATT_GRU_MAX_ENCODED = 4096, 320, 512


def att_gru_supported(T, A, E, H):
    """The limits of asr_att_gru_scan_*_f32 (include/asr_amd.h)."""
    return (1 <= T <= ATT_GRU_MAX_FRAMES and 1 <= A <= ATT_GRU_MAX_HIDDEN
            and 1 <= H <= ATT_GRU_MAX_HIDDEN and 1 <= E <= ATT_GRU_MAX_ENCODED
            and A % 4 == 0 and E % 4 == 0 and H % 4 == 0)


def att_gru_scan_fwd(eproj, encoded, enc_lens, gx_emb, w_ic, w_hh, b_hh, w_rec, w_score, b_score,
                     h0, beam=1, save=True):
    """asr_att_gru_scan_fwd_f32 -> (att [L, B, T], states [L, B, H], contexts [L, B, E],
    gates [L, B, 4H], rec [L, B, A]); the last three are None with save=False."""
    f32 = torch.float32
    eproj, encoded = _dev(eproj, f32, 'eproj'), _dev(encoded, f32, 'encoded')
    gx_emb, h0 = _dev(gx_emb, f32, 'gx_emb'), _dev(h0, f32, 'h0')
    w_ic, w_hh, b_hh = _dev(w_ic, f32, 'w_ic'), _dev(w_hh, f32, 'w_hh'), _dev(b_hh, f32, 'b_hh')
    w_rec, w_score = _dev(w_rec, f32, 'w_rec'), _dev(w_score, f32, 'w_score')
    b_score = _dev(b_score, f32, 'b_score')
    enc_lens = _dev(enc_lens, torch.int32, 'enc_lens')
    T, NU, A = eproj.shape
    E = encoded.shape[2]
    L, B, H3 = gx_emb.shape
    H = H3 // 3
    if (encoded.shape[:2] != (T, NU) or B != NU * beam or h0.shape != (B, H) or H3 != 3 * H
            or w_ic.shape != (H3, E) or w_hh.shape != (H3, H) or b_hh.numel() != H3
            or w_rec.shape != (A, H) or w_score.numel() != A or enc_lens.numel() != NU):
        raise AssertionError('asr_att_gru_scan_fwd_f32: inconsistent operand shapes')
    new = lambda *shape: torch.empty(shape, dtype=f32, device=eproj.device)  # noqa: E731
    att, states = new(L, B, T), new(L, B, H)
    ctxs, gates, rec = (new(L, B, E), new(L, B, 4 * H), new(L, B, A)) if save else (None,) * 3
    check(lib().asr_att_gru_scan_fwd_f32(
        _p(eproj), _p(encoded), _p(enc_lens), _p(gx_emb), _p(w_ic), _p(w_hh), _p(b_hh), _p(w_rec),
        _p(w_score), _p(b_score), _p(h0), T, B, beam, L, A, E, H, _p(att), _p(states), _p(ctxs),
        _p(gates), _p(rec), _stream()), 'asr_att_gru_scan_fwd_f32')
    return att, states, ctxs, gates, rec


def att_gru_scan_bwd(eproj, encoded, enc_lens, w_icT, w_hhT, w_recT, w_score, h0, att, states,
                     gates, rec, d_att, d_states):
    """asr_att_gru_scan_bwd_f32 -> (d_eproj [T, B, A], d_gates [L, B, 4H], d_contexts [L, B, E],
    d_rec [L, B, A], d_w_score partials [B, A], d_h0 [B, H]); d_att / d_states may be None."""
    f32 = torch.float32
    eproj, encoded = _dev(eproj, f32, 'eproj'), _dev(encoded, f32, 'encoded')
    w_icT, w_hhT = _dev(w_icT, f32, 'w_icT'), _dev(w_hhT, f32, 'w_hhT')
    w_recT, w_score = _dev(w_recT, f32, 'w_recT'), _dev(w_score, f32, 'w_score')
    h0, att, states = _dev(h0, f32, 'h0'), _dev(att, f32, 'att'), _dev(states, f32, 'states')
    gates, rec = _dev(gates, f32, 'gates'), _dev(rec, f32, 'rec')
    d_att = None if d_att is None else _dev(d_att, f32, 'd_att')
    d_states = None if d_states is None else _dev(d_states, f32, 'd_states')
    enc_lens = _dev(enc_lens, torch.int32, 'enc_lens')
    T, B, A = eproj.shape
    E = encoded.shape[2]
    L, _, H = states.shape
    if (encoded.shape[:2] != (T, B) or states.shape[1] != B or att.shape != (L, B, T)
            or gates.shape != (L, B, 4 * H) or rec.shape != (L, B, A) or h0.shape != (B, H)
            or w_icT.shape != (E, 3 * H) or w_hhT.shape != (H, 3 * H) or w_recT.shape != (H, A)
            or (d_att is not None and d_att.shape != att.shape)
            or (d_states is not None and d_states.shape != states.shape)):
        raise AssertionError('asr_att_gru_scan_bwd_f32: inconsistent operand shapes')
    dev = eproj.device
    d_eproj = torch.zeros_like(eproj)
    d_gates = torch.empty_like(gates)
    d_ctx = torch.empty((L, B, E), dtype=f32, device=dev)
    d_rec = torch.empty_like(rec)
    d_v = torch.empty((B, A), dtype=f32, device=dev)
    d_h0 = torch.empty_like(h0)
    check(lib().asr_att_gru_scan_bwd_f32(
        _p(eproj), _p(encoded), _p(enc_lens), _p(w_icT), _p(w_hhT), _p(w_recT), _p(w_score),
        _p(h0), _p(att), _p(states), _p(gates), _p(rec), _p(d_att), _p(d_states), T, B, L, A, E, H,
        _p(d_eproj), _p(d_gates), _p(d_ctx), _p(d_rec), _p(d_v), _p(d_h0), _stream()),
        'asr_att_gru_scan_bwd_f32')
    return d_eproj, d_gates, d_ctx, d_rec, d_v, d_h0


LM_BAG_CAP = 32


def beam_lm_supported(beam, C, bag_cap=LM_BAG_CAP):
    return bool(lib().asr_beam_lm_supported(beam, C, bag_cap))


def lm_label_costs(lm, bag_state, bag_cost, bag_n, mapping, frozen, B, beam, C, cost, bag_cap=LM_BAG_CAP):
    """asr_lm_label_costs_f64: `lm` = LmFst.device_arrays(); writes cost [B*beam, C] fp64."""
    check(lib().asr_lm_label_costs_f64(
        _p(lm['ptr']), _p(lm['ilabel']), _p(lm['w_closed']), lm['nstates'], _p(bag_state), _p(bag_cost),
        _p(bag_n), bag_cap, _p(mapping), _p(frozen), B, beam, C, _p(cost), _stream()),
        'asr_lm_label_costs_f64')
    return cost


def lm_bag_advance(lm, mapping, bags_in, bags_out, parent, new_input, nsteps, step, B, beam, overflow,
                   bag_cap=LM_BAG_CAP):
    """asr_lm_bag_advance_f64: bags_* = (state [hyps, cap] i32, cost [hyps, cap] f64, n [hyps] i32)."""
    check(lib().asr_lm_bag_advance_f64(
        _p(lm['ptr']), _p(lm['ptr_ne']), _p(lm['dst']), _p(lm['ilabel']), _p(lm['weight']), _p(lm['rank']),
        lm['nstates'], lm['max_rank'], _p(mapping), _p(bags_in[0]), _p(bags_in[1]), _p(bags_in[2]),
        _p(bags_out[0]), _p(bags_out[1]), _p(bags_out[2]), bag_cap, _p(parent), _p(new_input),
        _p(nsteps), step, B, beam, _p(overflow), _stream()), 'asr_lm_bag_advance_f64')


def beam_lm_step(logits, att, lens, lm_cost, lm_weight, scores_in, scores_out, est_in, est_out, cov_in,
                 cov_out, min_eos, step, B, beam, len_div, min_attention_pos, coverage_tau,
                 coverage_weight, state, fin_mask=None, tot_out=None):
    """asr_beam_lm_step_f32; `state` = dict of the per-utterance device arrays (fin_count, fin_parity,
    fin_score, fin_len, fin_beam, fin_tokens, best_score, best_len, best_tokens, best_elems,
    new_input, parent, frozen, nsteps).  With either of fin_mask [hyps] i32 / tot_out [hyps] f32
    given, asr_beam_lm_step_graph_f32: the same step plus those two outputs."""
    C, T = logits.shape[-1], att.shape[-1]
    graph = fin_mask is not None or tot_out is not None
    name = 'asr_beam_lm_step_graph_f32' if graph else 'asr_beam_lm_step_f32'
    extra = (_p(fin_mask), _p(tot_out)) if graph else ()
    check(getattr(lib(), name)(
        _p(logits), _p(att), _p(lens), _p(lm_cost), float(lm_weight), _p(scores_in), _p(scores_out),
        _p(est_in), _p(est_out), _p(cov_in), _p(cov_out), _p(min_eos), step, B, beam, C, T,
        est_in.shape[1], len_div, float(min_attention_pos), coverage_tau, coverage_weight,
        _p(state['fin_count']), _p(state['fin_parity']), _p(state['fin_score']), _p(state['fin_len']),
        _p(state['fin_beam']), _p(state['fin_tokens']), _p(state['best_score']), _p(state['best_len']),
        _p(state['best_tokens']), _p(state['best_elems']), _p(state['new_input']), _p(state['parent']),
        _p(state['frozen']), _p(state['nsteps']), *(extra + (_stream(),))), name)


beam_lm_step_graph = beam_lm_step       # positional callers: the same wrapper with both outputs given


def graph_search_supported(beam, span, T, bag_cap=LM_BAG_CAP):
    return bool(lib().asr_graph_search_supported(beam, span, T, bag_cap))


NODE_KEYS = ('node_count', 'node_score', 'node_len', 'node_tokens', 'node_att', 'node_bag_n',
             'node_bag_state', 'node_fin', 'node_uplink')


def graph_merge(att, lens, scores, tot, est_in, est_out, fin_mask, bags, nsteps, len_pow, step, B, beam,
                span, merge_threshold, store, bag_cap=LM_BAG_CAP):
    """asr_graph_merge_f32: `bags` = (state [hyps, cap] i32, cost, n [hyps] i32) of the survivors or
    None (no LM term); `store` = dict of the node arrays (NODE_KEYS) of include/asr_amd.h."""
    T, Lcap, Ncap = att.shape[-1], est_in.shape[1], store['node_score'].shape[1]
    check(lib().asr_graph_merge_f32(
        _p(att), _p(lens), _p(scores), _p(tot), _p(est_in), _p(est_out), _p(fin_mask),
        _p(bags[0]) if bags is not None else None, _p(bags[2]) if bags is not None else None, bag_cap,
        _p(nsteps), _p(len_pow), step, B, beam, T, Lcap, int(span), float(merge_threshold), Ncap,
        *([_p(store[k]) for k in NODE_KEYS] + [_stream()])), 'asr_graph_merge_f32')


def forced_level(logits, att, cov_in, cov_out, parent, edge_ptr, edge_label, edge_dst, acoustic_in,
                 acoustic_out, lens, B, width, coverage_tau, sent_acoustic, sent_covered):
    """asr_forced_level_f32: one trie level of the forced scorer.  logits [B*width, C], att / cov_out
    [B*width, T], cov_in [rows, T] indexed by parent [B*width]; edges in CSR form per slot; fp64
    acoustic carries; sent_acoustic fp64 / sent_covered i32 per sentence."""
    slots = B * width
    C, T = logits.shape[-1], att.shape[-1]
    assert logits.shape[0] == slots and att.shape[0] == slots and cov_out.shape[0] >= slots
    assert cov_in.shape[-1] == T and cov_out.shape[-1] == T and parent.numel() >= slots
    assert edge_ptr.numel() >= slots + 1 and acoustic_in.numel() >= slots
    assert edge_dst.numel() == edge_label.numel() and sent_covered.numel() == sent_acoustic.numel()
    check(lib().asr_forced_level_f32(
        _p(_dev(logits, torch.float32, 'logits')), _p(_dev(att, torch.float32, 'att')),
        _p(_dev(cov_in, torch.float32, 'cov_in')), _p(_dev(cov_out, torch.float32, 'cov_out')),
        _p(_dev(parent, torch.int32, 'parent')), _p(_dev(edge_ptr, torch.int32, 'edge_ptr')),
        _p(_dev(edge_label, torch.int32, 'edge_label')), _p(_dev(edge_dst, torch.int32, 'edge_dst')),
        _p(_dev(acoustic_in, torch.float64, 'acoustic_in')),
        _p(_dev(acoustic_out, torch.float64, 'acoustic_out')), _p(_dev(lens, torch.int32, 'lens')),
        B, width, C, T, cov_in.shape[0], edge_label.numel(), acoustic_out.numel(),
        sent_acoustic.numel(), float(coverage_tau), _p(_dev(sent_acoustic, torch.float64, 'sent_acoustic')),
        _p(_dev(sent_covered, torch.int32, 'sent_covered')), _stream()), 'asr_forced_level_f32')


def beam_step(logits, scores_in, scores_out, est_in, est_out, step, B, beam, len_div, state):
    """asr_beam_step_f32; `state` = dict of the per-utterance device arrays (finished_count,
    best_score, best_len, best_tokens, new_input, parent, done)."""
    C = logits.shape[-1]
    check(lib().asr_beam_step_f32(
        _p(logits), _p(scores_in), _p(scores_out), _p(est_in), _p(est_out), int(step), B, beam, C,
        est_in.shape[1], float(len_div), _p(state['finished_count']), _p(state['best_score']),
        _p(state['best_len']), _p(state['best_tokens']), _p(state['new_input']),
        _p(state['parent']), _p(state['done']), _stream()), 'asr_beam_step_f32')


def _nhwc_bf16(t, what):
    """logical [B, C, H, W] bf16 tensor in channels-last memory -> (tensor, B, C, H, W)"""
    if not t.is_cuda:
        raise NativeLibraryError("%s must live on the MI355X" % what)
    if t.dtype != torch.bfloat16:
        t = t.to(torch.bfloat16)
    t = t.contiguous(memory_format=torch.channels_last)
    return (t,) + tuple(t.shape)


def conv7x7c32_fwd(x, weight, stride_h, want_sums=False):
    """asr_conv7x7c32_fwd_bf16: x logical [B, 32, H, W] (channels-last bf16), weight
    [32, 32, 7, 7] f32 -> y logical [B, 32, Ho, Wo] channels-last bf16 (and, want_sums, the
    [2, 32] f64 channel sums / sums of squares of y for the following BatchNorm)."""
    x, B, C, H, W = _nhwc_bf16(x, 'x')
    weight = _dev(weight, torch.float32, 'weight')
    Ho, Wo = (H - 7) // stride_h + 1, W - 6
    y = torch.empty((B, 32, Ho, Wo), dtype=torch.bfloat16, device=x.device,
                    memory_format=torch.channels_last)
    L = lib()
    nbytes = L.asr_conv7x7c32_workspace_bytes()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    sums = torch.empty((2, 32), dtype=torch.float64, device=x.device) if want_sums else None
    check(L.asr_conv7x7c32_fwd_bf16(_p(x), _p(weight), B, H, W, int(stride_h), _p(y), _p(sums),
                                    _p(ws), nbytes, _stream()), 'asr_conv7x7c32_fwd_bf16')
    return (y, sums) if want_sums else y


def conv7x7c32_bwd_data(dy, weight, H, W, stride_h):
    """asr_conv7x7c32_bwd_data_bf16: dy logical [B, 32, Ho, Wo] -> dx logical [B, 32, H, W]
    (channels-last bf16)."""
    dy, B, C, Ho, Wo = _nhwc_bf16(dy, 'dy')
    weight = _dev(weight, torch.float32, 'weight')
    assert Ho == (H - 7) // stride_h + 1 and Wo == W - 6
    dx = torch.empty((B, 32, H, W), dtype=torch.bfloat16, device=dy.device,
                     memory_format=torch.channels_last)
    L = lib()
    nbytes = L.asr_conv7x7c32_workspace_bytes()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dy.device)
    check(L.asr_conv7x7c32_bwd_data_bf16(_p(dy), _p(weight), B, H, W, int(stride_h), _p(dx),
                                         _p(ws), nbytes, _stream()), 'asr_conv7x7c32_bwd_data_bf16')
    return dx


def conv7x7c32_wgrad(x, dy, stride_h):
    """asr_conv7x7c32_wgrad_bf16: x logical [B, 32, H, W], dy logical [B, 32, Ho, Wo]
    (channels-last bf16) -> dw [32, 32, 7, 7] f32."""
    x, B, C, H, W = _nhwc_bf16(x, 'x')
    dy = _nhwc_bf16(dy, 'dy')[0]
    dw = torch.empty((32, 32, 7, 7), dtype=torch.float32, device=x.device)
    L = lib()
    nbytes = L.asr_conv7x7c32_workspace_bytes()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    check(L.asr_conv7x7c32_wgrad_bf16(_p(x), _p(dy), B, H, W, int(stride_h), _p(dw), _p(ws),
                                      nbytes, _stream()), 'asr_conv7x7c32_wgrad_bf16')
    return dw


_INT_MAX = 2 ** 31 - 1


def conv7x7c32_supported(B, H, W, stride_h):
    """asr_conv7x7c32_supported: the shapes all three of asr_conv7x7c32_{fwd,bwd_data,wgrad}_bf16
    take (the launchers' own checks, so a shape claimed here is never answered with
    ASR_EUNSUPPORTED in the middle of a training step)"""
    B, H, W, stride_h = int(B), int(H), int(W), int(stride_h)
    if not (0 < B <= _INT_MAX and 0 < H <= _INT_MAX and 0 < W <= _INT_MAX and 0 < stride_h <= _INT_MAX):
        return False
    return bool(lib().asr_conv7x7c32_supported(B, H, W, stride_h))


def conv1_supported(F, cin):
    """asr_conv1_7x7s2_supported: the widths csrc/conv.hip has a first convolution for, forward
    and weight gradient both: one channel up to Fo = 39, or the WSJ recipes' 3 channels with an
    even output width up to Fo = 40"""
    F, cin = int(F), int(cin)
    return 7 <= F <= _INT_MAX and cin in (1, 3) and bool(lib().asr_conv1_7x7s2_supported(F, cin))


def conv1_fwd(x, weight, want_sums=False):
    """asr_conv1_7x7s2_fwd / asr_conv1c_7x7s2_fwd: x [B, T, F] or [B, T, F, cin] f32, weight
    [32, cin, 7, 7] f32 -> y logical [B, 32, T + 6, (F - 7) // 2 + 1] channels-last bf16."""
    x = _dev(x, torch.float32, 'x')
    weight = _dev(weight, torch.float32, 'weight')
    cin = x.shape[3] if x.dim() == 4 else 1
    B, T, F = x.shape[:3]
    if tuple(weight.shape) != (32, cin, 7, 7):
        raise ValueError('conv1_fwd: weight must be [32, %d, 7, 7]' % cin)
    y = torch.empty((B, 32, T + 6, (F - 7) // 2 + 1), dtype=torch.bfloat16, device=x.device,
                    memory_format=torch.channels_last)
    L = lib()
    sums = torch.empty((2, 32), dtype=torch.float64, device=x.device) if want_sums else None
    if cin == 1:
        nbytes = L.asr_conv1_7x7s2_workspace_bytes()
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        check(L.asr_conv1_7x7s2_fwd(_p(x), _p(weight), B, T, F, _p(y), _p(sums), _p(ws), nbytes,
                                    _stream()), 'asr_conv1_7x7s2_fwd')
    else:
        nbytes = L.asr_conv1c_7x7s2_workspace_bytes(cin)
        if nbytes < 0:
            raise NotImplementedError('conv1_fwd: %d input channels' % cin)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        check(L.asr_conv1c_7x7s2_fwd(_p(x), _p(weight), B, T, F, cin, _p(y), _p(sums), _p(ws), nbytes,
                                     _stream()), 'asr_conv1c_7x7s2_fwd')
    return (y, sums) if want_sums else y


def conv1_wgrad(x, dy):
    """asr_conv1_7x7s2_wgrad / asr_conv1c_7x7s2_wgrad: x [B, T, F] or [B, T, F, cin] f32, dy
    logical [B, 32, To, Fo] channels-last bf16 -> dw [32, cin, 7, 7] f32."""
    x = _dev(x, torch.float32, 'x')
    dy = _nhwc_bf16(dy, 'dy')[0]
    cin = x.shape[3] if x.dim() == 4 else 1
    B, T, F = x.shape[:3]
    dw = torch.empty((32, cin, 7, 7), dtype=torch.float32, device=x.device)
    L = lib()
    if cin == 1:
        nbytes = L.asr_conv1_7x7s2_workspace_bytes()
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        check(L.asr_conv1_7x7s2_wgrad(_p(x), _p(dy), B, T, F, _p(dw), _p(ws), nbytes, _stream()),
              'asr_conv1_7x7s2_wgrad')
    else:
        nbytes = L.asr_conv1c_7x7s2_workspace_bytes(cin)
        if nbytes < 0:
            raise NotImplementedError('conv1_wgrad: %d input channels' % cin)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        check(L.asr_conv1c_7x7s2_wgrad(_p(x), _p(dy), B, T, F, cin, _p(dw), _p(ws), nbytes, _stream()),
              'asr_conv1c_7x7s2_wgrad')
    return dw


def conv1_wgrad_bn_supported(F, cin=1):
    """widths asr_conv1_7x7s2_wgrad_bn is built for (one input channel)"""
    return cin == 1 and F >= 7 and bool(lib().asr_conv1_7x7s2_wgrad_bn_supported(int(F)))


def conv1_wgrad_bn(x, z, dy, conv_bias, gamma, beta, mean, invstd, training, lo, hi, bn_ws, n_total):
    """asr_conv1_7x7s2_wgrad_bn: x [B, T, F] f32, z (the convolution's output) and dy (the
    gradient reaching the BatchNorm + Hardtanh's output) logical [B, 32, To, Fo] channels-last
    bf16, bn_ws the workspace bn_act_bwd_sums left (its sums possibly all-reduced, standing for
    n_total elements) -> dw [32, 1, 7, 7] f32: the weight gradient with the BatchNorm backward
    applied on the way in, bit for bit bn_act_bwd's dx fed to conv1_wgrad."""
    x = _dev(x, torch.float32, 'x')
    if z.dtype != torch.bfloat16 or dy.dtype != torch.bfloat16:
        raise TypeError('conv1_wgrad_bn: z and dy must be bfloat16')
    z = _nhwc_bf16(z, 'z')[0]
    dy = _nhwc_bf16(dy, 'dy')[0]
    B, T, F = x.shape
    if tuple(z.shape) != (B, 32, T + 6, (F - 7) // 2 + 1) or z.shape != dy.shape:
        raise ValueError('conv1_wgrad_bn: z / dy must be [%d, 32, %d, %d]' % (B, T + 6, (F - 7) // 2 + 1))
    if conv_bias is not None:
        conv_bias = _dev(conv_bias, torch.float32, 'conv_bias')
    dw = torch.empty((32, 1, 7, 7), dtype=torch.float32, device=x.device)
    L = lib()
    nbytes = L.asr_conv1_7x7s2_workspace_bytes()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    check(L.asr_conv1_7x7s2_wgrad_bn(
        _p(x), _p(z), _p(dy), B, T, F, _p(conv_bias), _p(_dev(gamma, torch.float32, 'gamma')),
        _p(_dev(beta, torch.float32, 'beta')), _p(mean), _p(invstd), int(bool(training)),
        float(lo), float(hi), _p(bn_ws), float(n_total), _p(dw), _p(ws), nbytes, _stream()),
        'asr_conv1_7x7s2_wgrad_bn')
    return dw


def split_bf16(x, hi=None, lo=None):
    """asr_split_bf16_f32: x f32 on the GPU -> (hi, lo) bf16 with hi + lo = x to 2^-16.
    x contiguous of any shape (new contiguous outputs), or x [rows, cols] with given 2-D
    output views hi / lo whose last dimension is dense (the halves of a K-concatenated
    GEMM operand)."""
    x = _dev(x, torch.float32, 'x')
    if hi is None:
        hi = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
        lo = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
        rows, cols, ldx, ldh, ldl = 1, x.numel(), x.numel(), x.numel(), x.numel()
    else:
        if x.dim() != 2 or hi.shape != x.shape or lo.shape != x.shape or x.stride(1) != 1 \
                or hi.stride(1) != 1 or lo.stride(1) != 1 or hi.dtype != torch.bfloat16 or lo.dtype != torch.bfloat16:
            raise ValueError('split_bf16: x, hi, lo must be [rows, cols] with a dense last dimension')
        rows, cols = x.shape
        ldx, ldh, ldl = x.stride(0), hi.stride(0), lo.stride(0)
    check(lib().asr_split_bf16_f32(_p(x), rows, cols, ldx, _p(hi), ldh, _p(lo), ldl, _stream()),
          'asr_split_bf16_f32')
    return hi, lo


def sum_leading(t):
    """asr_sum_leading_f32: t [G, ...] f32 contiguous on the GPU -> t.sum(0); torch's own sum for
    what the kernel does not take (n % 4 != 0, a view that does not start on 16 bytes)"""
    if not t.is_cuda or t.dtype != torch.float32 or (t[0].numel() & 3):
        return t.sum(0)
    t = t.contiguous()
    if t.data_ptr() & 15:
        return t.sum(0)
    out = torch.empty(t.shape[1:], dtype=torch.float32, device=t.device)
    check(lib().asr_sum_leading_f32(_p(t), t.shape[0], t[0].numel(), _p(out), _stream()),
          'asr_sum_leading_f32')
    return out


def log_softmax_shift_fwd(x, lens):
    """asr_log_softmax_shift_fwd_f32: x [T, B, C] -> (y = x - max_c x, nls [T, B], nls_sum [B])"""
    x = _dev(x, torch.float32, 'logits')
    lens = _dev(lens, torch.int32, 'lens')
    T, B, C = x.shape
    y = torch.empty_like(x)
    nls = torch.empty((T, B), dtype=torch.float32, device=x.device)
    nls_sum = torch.empty(B, dtype=torch.float32, device=x.device)
    check(lib().asr_log_softmax_shift_fwd_f32(_p(x), T, B, C, _p(lens), _p(y), _p(nls), _p(nls_sum),
                                              _stream()), 'asr_log_softmax_shift_fwd_f32')
    return y, nls, nls_sum


def log_softmax_shift_bwd_split(y, nls, dy, ld):
    """asr_log_softmax_shift_bwd_split_bf16: the gradient of log_softmax_shift_fwd as bf16
    halves (hi, lo) [rows, ld] (columns >= C zero) and its column sums [C]."""
    y, dy = _dev(y, torch.float32, 'y'), _dev(dy, torch.float32, 'dy')
    C = y.shape[-1]
    rows = y.numel() // C
    L = lib()
    hi = torch.empty((rows, ld), dtype=torch.bfloat16, device=y.device)
    lo = torch.empty((rows, ld), dtype=torch.bfloat16, device=y.device)
    part = torch.empty((L.asr_log_softmax_shift_bwd_split_blocks(rows), ld), dtype=torch.float32, device=y.device)
    check(L.asr_log_softmax_shift_bwd_split_bf16(_p(y), _p(nls), _p(dy), rows, C, _p(hi), _p(lo), int(ld),
                                                 _p(part), _stream()), 'asr_log_softmax_shift_bwd_split_bf16')
    nb = part.shape[0]
    if nb % 32 == 0 and nb > 32:         # two stages: sum_leading walks its leading axis serially
        part = sum_leading(part.view(32, (nb // 32) * ld)).view(nb // 32, ld)
    return hi, lo, sum_leading(part)[:C]


def log_softmax_shift_bwd(y, nls, dy):
    y, dy = _dev(y, torch.float32, 'y'), _dev(dy, torch.float32, 'dy')
    C = y.shape[-1]
    dx = torch.empty_like(y)
    check(lib().asr_log_softmax_shift_bwd_f32(_p(y), _p(nls), _p(dy), y.numel() // C, C, _p(dx),
                                              _stream()), 'asr_log_softmax_shift_bwd_f32')
    return dx


def edit_distance_max_len():
    """asr_edit_distance_max_len: the longest side asr_edit_distance_stats_i32 is built for."""
    return int(lib().asr_edit_distance_max_len())


def edit_distance_stats(x, x_off, y, y_off, max_x, max_y):
    """asr_edit_distance_stats_i32: flat int32 token ids x, y with prefix offsets x_off, y_off
    [n + 1] (all on the GPU; max_x, max_y: host bounds of the pairs' lengths) -> int32 [n, 4]
    (dist, ins, del, sub) per pair.  Lengths above edit_distance_max_len() are refused
    (AssertionError) before anything is launched."""
    x, x_off = _dev(x, torch.int32, 'x'), _dev(x_off, torch.int32, 'x_off')
    y, y_off = _dev(y, torch.int32, 'y'), _dev(y_off, torch.int32, 'y_off')
    n = x_off.numel() - 1
    if n < 0 or y_off.numel() != n + 1:
        raise AssertionError('edit_distance_stats: x_off and y_off must both hold n + 1 offsets')
    out = torch.empty((n, 4), dtype=torch.int32, device=x.device)
    check(lib().asr_edit_distance_stats_i32(_p(x), _p(x_off), _p(y), _p(y_off), n, int(max_x),
                                            int(max_y), _p(out), _stream()),
          'asr_edit_distance_stats_i32')
    return out


def ctc_align_supported(T, Lmax, C):
    """asr_ctc_align_supported: whether asr_ctc_align_f64 is built for these shapes."""
    return bool(lib().asr_ctc_align_supported(int(T), int(Lmax), int(C)))


def ctc_align(lp, lens, labels, label_lens, num_symbols, context_order=1,
              allow_nonblank_selfloops=True, eval_repeats_in_context=False):
    """asr_ctc_align_f64: lp [T, B, C] f32 (finite), lens [B] i32, labels [B, Lmax] i32, label_lens
    [B] i32, all on the GPU -> (cost [B] f64, frames [B, T] i32, states [B, T] i32, segments
    [B, Lmax, 2] i32), one launch for the batch.  Shapes the kernel is not built for raise
    NotImplementedError before anything is launched."""
    lp = _dev(lp, torch.float32, 'log_probs')
    lens, label_lens = _dev(lens, torch.int32, 'lens'), _dev(label_lens, torch.int32, 'label_lens')
    labels = _dev(labels, torch.int32, 'labels')
    T, B, C = lp.shape
    Lmax = labels.shape[1] if labels.dim() == 2 else -1
    if Lmax < 0 or labels.shape[0] != B or lens.numel() != B or label_lens.numel() != B:
        raise AssertionError('ctc_align: lens [B], labels [B, Lmax] and label_lens [B] must match lp [T, B, C]')
    L = lib()
    dev = lp.device
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    frames = torch.empty((B, T), dtype=torch.int32, device=dev)
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    segments = torch.empty((B, Lmax, 2), dtype=torch.int32, device=dev)
    nbytes = int(L.asr_ctc_align_workspace_bytes(T, B, Lmax))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    check(L.asr_ctc_align_f64(_p(lp), _p(lens), _p(labels), _p(label_lens), B, T, C, Lmax,
                              int(num_symbols), int(context_order), int(bool(allow_nonblank_selfloops)),
                              int(bool(eval_repeats_in_context)), _p(cost), _p(frames), _p(states),
                              _p(segments), _p(ws), nbytes, _stream()), 'asr_ctc_align_f64')
    return cost, frames, states, segments
