#!/usr/bin/env python3
"""np.array_equal of every array two `bench.py --dump-outputs` runs left behind (two builds of the library, same command).
  python tools/compare_outputs.py DIR_A DIR_B   -> one line per array, then ALL IDENTICAL or DIFFERENT; exit status 1 if any differs"""
import os
import sys

import numpy as np

a, b = sys.argv[1:3]
names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
assert names and names == sorted(f for f in os.listdir(b) if f.endswith(".npy")), (names, os.listdir(b))
ok = True
for f in names:
    x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
    same = x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))   # bits: NaNs and signed zeros count
    ok &= same
    print(f"{f:20s} {str(x.dtype):8s} {str(x.shape):14s} nonzero={int(np.count_nonzero(x))} {'IDENTICAL' if same else 'DIFFERENT'}")
print("ALL IDENTICAL" if ok else "DIFFERENT")
sys.exit(0 if ok else 1)
