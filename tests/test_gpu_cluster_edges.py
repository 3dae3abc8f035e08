# coding=utf-8
"""-m gpu: stage A0 at the named plan, tile and size-class boundaries of its host driver and kernels (tests/cluster_cases.py;
tests/test_cluster_case_edges.py shows on the CPU that every case sits on its edge; DESIGN.md section 22 has the table).  Each
case goes through Context.cluster_host in every (hints, debug word) combination of test_gpu_cluster.MODES -- the cases of 65,000
marks and more in the subset cluster_cases.SUBSET names -- and is compared with oracle.c_oracle.cluster field for field, exactly."""
import pytest

from duet_amd import _lib
from tests import cluster_cases as C
from tests.test_gpu_cluster import MODES, check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.set_debug(0)
    c.close()


@pytest.mark.parametrize('name', C.NAMES)
def test_case_matches_the_oracle(ctx, name):
    marks, kw = C.case(name)
    check(ctx, marks, modes=C.SUBSET.get(name, MODES), **kw)
