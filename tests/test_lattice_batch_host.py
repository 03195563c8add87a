"""csrc/lattice_batch.h, the header the lattice kernels share, on the CPU: tests/lattice_batch_host.cpp is built
host-only with AddressSanitizer and UBSan and run as a program of its own (no GPU, no Python extension).  Its
batch lives in heap arrays of exactly the batch's sizes, so a helper that used an index before checking it
would end the run with a sanitizer report."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, 'lattice_batch_host.cpp')


def cpu_has_fma():
    try:
        with open('/proc/cpuinfo') as f:
            return any(line.startswith('flags') and ' fma ' in line + ' ' for line in f)
    except OSError:
        return False


def compiler():
    """the HIP compiler the library is built with, host side only; else the system's C++ compiler"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if os.path.exists(hipcc) or shutil.which(hipcc):
        flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
        if cpu_has_fma():       # let the compiler fuse where it may: arc_cost's pragma must then hold on its own
            flags += ['-mfma', '-ffp-contract=fast-honor-pragmas']
        return [hipcc, '--offload-host-only', '-x', 'hip'] + [x for f in flags for x in ('-Xarch_host', f)]
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    assert cxx, "no hipcc and no C++ compiler"
    return [cxx, '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']


def test_the_header_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'lattice_batch_host')
    build = subprocess.run(compiler() + ['-std=c++17', '-O1', '-g', '-Wall', '-Wno-unused-function', SOURCE, '-o', exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert run.stdout.strip().endswith('lattice_batch_host ok') and 'runtime error' not in run.stderr, run.stderr
