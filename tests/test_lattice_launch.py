"""What the six lattice DP operations of att_speech.lattice_dp share, as far as a machine without a GPU can see it:
the ctypes signatures of their entry points against the declarations of include/asr_amd.h, position by position, the
check that keeps DeviceLatticeBatch.ilabel from gathering by a graph arc outside the graph, and the launch count of a
fresh batch."""
import ctypes
import os
import re

import pytest

import nbest_cases

from att_speech import _native
from att_speech.lattice_dp import DeviceLatticeBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('asr_lattice_bestpath_f64', 'asr_lattice_posterior_f64', 'asr_lattice_nbest_f64', 'asr_lattice_mbr_f64',
           'asr_lattice_oracle_i32', 'asr_lattice_seqtrain_f64')
KINDS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'double': ctypes.c_double}


def declared_kinds(header, name):
    """the ctypes kind of every parameter of `int name(...);` in the header: a pointer, or int / int64_t / double"""
    params = re.search(r'\bint %s\(([^;]*)\);' % name, header).group(1).split(',')
    kinds = []
    for param in params:
        words = param.replace('*', ' * ').split()
        assert len(words) >= 2, param                           # a type and a name at the least
        kinds.append(ctypes.c_void_p if '*' in words else KINDS[' '.join(w for w in words[:-1] if w != 'const')])
    return kinds


@pytest.mark.parametrize('name', ENTRIES)
def test_signature_is_the_headers(name):
    header = open(os.path.join(ROOT, 'include', 'asr_amd.h')).read()
    restype, argtypes = _native._SIGNATURES[name]
    want = declared_kinds(header, name)
    assert restype is ctypes.c_int and len(argtypes) == len(want)
    for i, (got, kind) in enumerate(zip(argtypes, want)):
        assert got is kind, (name, i, got, kind)


def toy_batch():
    return DeviceLatticeBatch.from_lattices(nbest_cases.toy_lattices('a', 1.0, 2.0)[0], 'cpu')


def test_a_fresh_batch_has_launched_nothing():
    assert toy_batch().launches == 0


@pytest.mark.parametrize('value', (10 ** 6, -1))
def test_ilabel_refuses_an_arc_outside_the_graph(value):
    """an unchecked gather on the CPU raises IndexError (10 ** 6) or wraps round (-1): ValueError shows that the
    check ran before the index"""
    T, C = 5, 3                                                 # the toys' scores: nbest_cases.toy_inputs
    good = toy_batch()
    assert len(good.ilabel) == good.num_arcs and len(good.depth()) == good.num_utterances
    assert good._emission_index(T, C)['E'] > 0
    for use in (lambda b: b.ilabel, lambda b: b.depth(), lambda b: b._emission_index(T, C)):
        batch = toy_batch()
        batch.arc[1] = value
        with pytest.raises(ValueError, match='outside the graph'):
            use(batch)
