#!/usr/bin/env python
"""Generates ``tests/golden/reference_outputs_golden.npz``: the reference's outputs (its own classes executed on CPU
through oracle/ref_import.py, and the settings of its config files) that the CPU tests compare with, recorded by
``tests/reference_record.py`` while those tests run in record mode.

Run where the reference tree is present:

    python tests/golden/make_golden_reference_outputs.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TESTS = ['tests/test_detector_host_cpu.py', 'tests/test_cascade_cpu.py', 'tests/test_htc_cpu.py',
         'tests/test_mask_cpu.py', 'tests/test_formats_cpu.py', 'tests/test_boundary_cpu.py']


def main():
    sys.path.insert(0, ROOT)
    from oracle import ref_import
    assert ref_import.reference_available(), 'needs the reference tree'
    env = dict(os.environ, BGS_RECORD_REFERENCE='1')
    sys.exit(subprocess.call([sys.executable, '-m', 'pytest', '-q', '-p', 'no:cacheprovider'] + TESTS,
                             cwd=ROOT, env=env))


if __name__ == '__main__':
    main()
