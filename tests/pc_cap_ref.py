# coding=utf-8
"""Test-side reference for the PC cap as a run parameter (duet_amd/csrc/duet_tune_cap.hip, `--pc_cap`): tests/tune_ref.py's
restatements with oracle.ef_oracle.PC_MAX set to the cap for the duration of one call.  seed_ps and vote are the only two
functions of the oracle that read the constant, and they read it at call time; the oracle file itself stays as it is.
demote() ties the parameterised reference back to the unpatched oracle: for a cap at or below 8100, raising every pc in
(cap, 8100] to 8101 gives the problem whose features under the reference's own cap are the features under `cap`."""
import numpy as np

from duet_amd import engine
from oracle import ef_oracle as O
from tests import tune_ref


class _cap(object):
    def __init__(self, cap):
        self.cap = int(cap)

    def __enter__(self):
        self.old = O.PC_MAX
        O.PC_MAX = self.cap

    def __exit__(self, *exc):
        O.PC_MAX = self.old


def features(soa, svlen_thres, suppread_thres, cap):
    """tune_ref.oracle_features under PC cap `cap`."""
    with _cap(cap):
        return tune_ref.oracle_features(soa, svlen_thres, suppread_thres)


def phased_text(home, svlen_thres, suppread_thres, vec, cap, include_all_ctgs=False):
    """tune_ref.phased_text under PC cap `cap`."""
    with _cap(cap):
        return tune_ref.phased_text(home, svlen_thres, suppread_thres, vec, include_all_ctgs)


def demote(soa, cap):
    """A copy of soa whose tag words have every pc in (cap, 8100] replaced by 8101."""
    tag = soa.read_tag.copy()
    pc = (tag >> np.uint64(32)) & np.uint64(0x3FFFFFFF)
    hit = (pc > np.uint64(int(cap))) & (pc <= np.uint64(8100))
    tag[hit] = (tag[hit] & ~(np.uint64(0x3FFFFFFF) << np.uint64(32))) | (np.uint64(8101) << np.uint64(32))
    kw = {name: getattr(soa, name).copy() for name, _ in engine.EfSoA.FIELDS}
    kw['read_tag'] = tag
    return engine.EfSoA(read_off=soa.read_off.copy(), **kw)
