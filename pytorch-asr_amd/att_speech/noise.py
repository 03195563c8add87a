"""Counter-based Gaussian noise on the device (csrc/noise.hip, include/asr_amd.h:
asr_gaussian_noise_f32) for the weight- and gradient-noise hooks.

z[i] is a function of (seed, tag, iteration, global index i) only, so the pass that removes
weight noise regenerates what the first pass added, and every rank of a data-parallel run draws
the same noise (the reference's `randn_like` draws from each process's own generator).
`philox4x32_10` / `normal_f64` below are the numpy statement of the same draw that the tests
check the kernel against.

The torch fallback (CPU tensors, other dtypes, ASR_NATIVE_NOISE=0) draws from a
`torch.Generator` seeded from (seed, tag, iteration): the same on every rank too, but not the
same numbers as the kernel."""
import os

import numpy as np
import torch
import torch.distributed as dist

TAG_WEIGHT, TAG_GRADIENT = 0, 1
APPLY, WRITE = 0, 1           # ASR_NOISE_APPLY, ASR_NOISE_WRITE

SEGMENT = np.dtype([('data', '<u8'), ('index', '<u8'), ('count', '<u4'), ('sigma', '<f4')])


def native_enabled():
    """ASR_NATIVE_NOISE=0 sends the noise hooks to their torch path (default: the kernel)."""
    return os.environ.get('ASR_NATIVE_NOISE', '1') != '0'


def native_ok(tensors):
    """The kernel takes contiguous fp32 GPU memory on one device."""
    if not tensors or not native_enabled():
        return False
    dev = tensors[0].device
    return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev
               for t in tensors)


# ---------------------------------------------------------------------------------------------
# the seed
# ---------------------------------------------------------------------------------------------
def draw_seed(group=None):
    """A 63-bit seed from the CPU default generator; under torch.distributed with world > 1, rank
    0's value broadcast to every rank (one collective)."""
    seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)
    seed = seed * 2 + torch.randint(0, 2, (1,), dtype=torch.int64)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        t = seed
        if dist.get_backend(group) == 'nccl':
            t = seed.cuda()
        dist.broadcast(t, src=0, group=group)
        seed = t.cpu()
    return int(seed.item())


# ---------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------
class SegmentTable(object):
    """Device table of (address, global index, count, sigma) pieces over a list of tensors whose
    global indices are given.  The pieces are cut again when an address moves; a change of the
    sigmas alone (LinearIncreaseWeightNoise's ramp) only refills that column and uploads the
    table through pinned memory, without waiting for the device."""

    def __init__(self):
        self._layout_key = None
        self._rows = None           # numpy SEGMENT rows of the current layout, sigma unset
        self._owner = None          # tensor number of every row
        self._sig_key = None
        self.table = None
        self.nsegs = 0

    def _layout(self, tensors, starts):
        key = (tuple(t.data_ptr() for t in tensors), tuple(starts))
        if key == self._layout_key:
            return
        from att_speech import _native
        ce = _native.lib().asr_noise_chunk_elems()
        data, index, count, owner = [], [], [], []
        for k, (t, i0) in enumerate(zip(tensors, starts)):
            n, base = t.numel(), t.data_ptr()
            if i0 + n >= 1 << 34:
                raise ValueError('global noise index beyond 2^34')
            for o in range(0, n, ce):
                data.append(base + 4 * o)
                index.append(i0 + o)
                count.append(min(ce, n - o))
                owner.append(k)
        self._rows = np.zeros(len(data), dtype=SEGMENT)
        self._rows['data'], self._rows['index'], self._rows['count'] = data, index, count
        self._owner = np.asarray(owner, dtype=np.int64)
        self._layout_key = key
        self._sig_key = None

    def get(self, tensors, starts, sigmas):
        self._layout(tensors, starts)
        sig_key = tuple(float(s) for s in sigmas)
        if sig_key == self._sig_key:
            return self.table, self.nsegs
        sig = np.asarray(sig_key, dtype=np.float32)[self._owner] if len(self._owner) else \
            np.zeros(0, np.float32)
        keep = sig != 0                         # nothing to add: no segment
        rows = self._rows[keep].copy()
        rows['sigma'] = sig[keep]
        self.nsegs = len(rows)
        self.table = None
        if self.nsegs:
            host = torch.from_numpy(rows.view(np.uint8).copy())
            dev = tensors[0].device
            if dev.type == 'cuda':
                host = host.pin_memory()
            self.table = host.to(dev, non_blocking=True)
        self._sig_key = sig_key
        return self.table, self.nsegs


def launch(table, nsegs, seed, tag, iteration, mode=APPLY, sign=1):
    """One asr_gaussian_noise_f32 over a SegmentTable's device table (nothing when it is empty)."""
    if nsegs == 0:
        return
    from att_speech import _native
    L = _native.lib()
    _native.check(L.asr_gaussian_noise_f32(_native._p(table), nsegs, seed % (1 << 64), int(tag),
                                           int(iteration) % (1 << 64), int(mode), int(sign),
                                           _native._stream()), 'asr_gaussian_noise_f32')


def write_normal(tensors, starts, seed, tag, iteration):
    """tensors[k] = z over global indices starts[k] .. (the tests' view of the draw)."""
    tab = SegmentTable()
    table, nsegs = tab.get(tensors, starts, [1.0] * len(tensors))
    launch(table, nsegs, seed, tag, iteration, mode=WRITE)


# ---------------------------------------------------------------------------------------------
# the torch fallback
# ---------------------------------------------------------------------------------------------
def torch_generator(device, seed, tag, iteration):
    g = torch.Generator(device=device)
    g.manual_seed((seed * 0x9E3779B97F4A7C15 + tag * 0xBF58476D1CE4E5B9 + iteration) % (1 << 63))
    return g


# ---------------------------------------------------------------------------------------------
# numpy statement of the draw (float64 Box-Muller on the same uniforms)
# ---------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: uint array [..., 4], key: uint array [..., 2] -> uint32 [..., 4] (Random123)."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., j] for j in range(4)]
    k0 = np.asarray(key, dtype=np.uint64)[..., 0].copy()
    k1 = np.asarray(key, dtype=np.uint64)[..., 1].copy()
    for r in range(10):
        if r:
            k0 = (k0 + _W0) & _MASK
            k1 = (k1 + _W1) & _MASK
        p0 = c[0] * np.uint64(_M0)
        p1 = c[2] * np.uint64(_M1)
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(_MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(_MASK)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return np.stack(c, -1).astype(np.uint32)


def normal_f64(indices, seed, tag, iteration):
    """z[i] in float64 for the global indices `indices` (the kernel's value up to fp32 rounding)."""
    idx = np.asarray(indices, dtype=np.uint64)
    g = idx >> np.uint64(2)
    ctr = np.stack([g & np.uint64(_MASK), np.full_like(g, tag),
                    np.full_like(g, iteration & _MASK), np.full_like(g, (iteration >> 32) & _MASK)], -1)
    key = np.broadcast_to(np.array([seed & _MASK, (seed >> 32) & _MASK], dtype=np.uint64), ctr.shape[:-1] + (2,))
    x = philox4x32_10(ctr, key).astype(np.float64)
    u = np.floor(x / 512.0) * 2.0 ** -23 + 2.0 ** -24
    j = (idx & np.uint64(3)).astype(np.int64)
    pair = j // 2
    ua = np.take_along_axis(u, (2 * pair)[:, None], 1)[:, 0]
    ub = np.take_along_axis(u, (2 * pair + 1)[:, None], 1)[:, 0]
    r = np.sqrt(-2.0 * np.log(ua))
    return np.where(j % 2 == 0, r * np.cos(2 * np.pi * ub), r * np.sin(2 * np.pi * ub))
