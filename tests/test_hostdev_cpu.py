"""The buffer owner the file path's device stages share (csrc/pcabi_hostdev.h), without a GPU:
tests/hostdev_main.cpp drives Owned over a fake memory policy that counts live blocks and fails an
allocation on request -- reserve within the capacity, growth, a failed reserve and its retry, moves
and destruction, and a stage of several owners whose third allocation fails (the stages' "do the kept
buffers serve" test must then say no). Built with -fsanitize=address,undefined as a program of its
own and run as a child process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_owner_under_sanitizers(tmp_path):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'hostdev')
    base = ['g++', '-O1', '-g', '-std=c++17', '-Wall', '-pthread', '-fsanitize=address,undefined',
            '-fno-sanitize-recover=all', '-o', exe, os.path.join(HERE, 'hostdev_main.cpp')]
    for extra in (['-static-libasan', '-static-libubsan'], []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    if r.returncode != 0 and ('asan' in r.stderr or 'ubsan' in r.stderr or 'sanitize' in r.stderr):
        pytest.skip('the sanitizer runtime cannot be linked')
    assert r.returncode == 0, r.stderr
    assert 'warning' not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'hostdev ok' in r.stdout
