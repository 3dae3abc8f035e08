# coding=utf-8
"""What the device primitives of duet_amd/csrc/duet_prims.hip.h compute, in numpy (tests/test_prims_ref_host.py checks these on
hand-written inputs; tests/test_gpu_prims.py compares the kernels with them, exactly)."""
import numpy as np


def sort_ref(keys, vals=None, key_bits=64, first_shift=0):
    """radix_sort_pairs: the stable order of the key bits [first_shift, key_bits); the whole 64-bit keys (and the values) travel.
    -> (keys[order], vals[order] or None)"""
    keys = np.asarray(keys, dtype=np.uint64)
    mask = (1 << (int(key_bits) - int(first_shift))) - 1                 # a Python integer: exact for 64 bits
    digits = (keys >> np.uint64(first_shift)) & np.uint64(mask)
    if mask < (1 << 16):
        digits = digits.astype(np.uint16)                                # (the same order; numpy's stable sort of 16 bits is a radix sort)
    order = np.argsort(digits, kind='stable')
    return keys[order], (None if vals is None else np.asarray(vals, dtype=np.uint32)[order])


def local_sort_ref(keys, key_bits):
    """global passes + rx_local + rx_big: the stable order of the low key_bits"""
    return sort_ref(keys, None, key_bits, 0)[0]


def scan_ref(values, op, n_dyn=None, prefill=0xA5A5A5A5):
    """launch_scan: op 0 the exclusive sum mod 2^32, op 1 the inclusive maximum, over the first min(n, n_dyn) elements; out behind
    them keeps the prefill.  -> (out u32[n], total)"""
    values = np.asarray(values, dtype=np.uint32)
    n = len(values)
    m = n if n_dyn is None else min(n, int(n_dyn))
    out = np.full(n, prefill, dtype=np.uint32)
    if m == 0:
        return out, 0
    if op == 0:
        inc = np.cumsum(values[:m], dtype=np.uint32)                     # wraps mod 2^32: the specified behaviour
        out[0] = 0
        out[1:m] = inc[:m - 1]
        return out, int(inc[m - 1])
    inc = np.maximum.accumulate(values[:m])
    out[:m] = inc
    return out, int(inc[m - 1])
