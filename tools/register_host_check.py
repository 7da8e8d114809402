#!/usr/bin/env python3
"""Builds tools/register_host_check.cpp (the argument checks of apq_rigid_register, csrc/seq/seq_register_checks.h, compiled
for the host) with -fsanitize=address,undefined and runs it: every served corner and every refusal, by name, on addresses
inside and beside real allocations.  A stand-alone program; nothing of it is loaded into Python.

    python tools/register_host_check.py [--cxx g++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cxx', default='g++')
    args = ap.parse_args()
    exe = os.path.join(tempfile.mkdtemp(), 'register_host_check')
    subprocess.check_call([args.cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(ROOT, 'tools', 'register_host_check.cpp'), '-o', exe])
    return subprocess.call([exe])


if __name__ == '__main__':
    sys.exit(main())
