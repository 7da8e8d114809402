#!/usr/bin/env python3
"""Builds tools/style_host_check.cpp (the argument checks and launch planners of libapstyle.so, compiled for the host from
csrc/style/style_checks.h) with -fsanitize=address,undefined and runs it: a sweep of every call over the corners of its served
region and past each limit.  No device is involved.

    python tools/style_host_check.py [--cxx g++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(work, cxx='g++'):
    exe = os.path.join(work, 'style_host_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(ROOT, 'tools', 'style_host_check.cpp'), '-o', exe])
    return exe


def run(cxx='g++'):
    """The program's last line; raises when it reports a failure or a sanitiser stops it."""
    with tempfile.TemporaryDirectory() as work:
        out = subprocess.run([build(work, cxx)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if out.returncode != 0:
        raise RuntimeError('style_host_check failed (%d):\n%s%s' % (out.returncode, out.stdout, out.stderr))
    return out.stdout.strip().splitlines()[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cxx', default='g++')
    print(run(ap.parse_args().cxx))
    return 0


if __name__ == '__main__':
    sys.exit(main())
