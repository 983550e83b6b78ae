"""Exact tests of the S3 native data plane with a device attached (real MI355X).

Every case of tests/test_s3_dataplane_exact.py - see there for the contract and
the oracle - runs here with dev = 0: the plane chunks the body over its 2-slot
ring, PUT bodies come from the fill kernel through D2H, GET bodies go through
H2D into the async verify kernel, body_crc reduces in HBM, and the chunks the
kernels do not take (ragged length, misaligned offset) fall to the host.

On top of that, PUT bodies of a plane with a device and one without are
compared with each other.
"""

import pytest

# the cases, their fixtures and helpers; `dev` is overridden below
from tests.test_s3_dataplane_exact import *  # noqa: F401,F403
from tests.test_s3_dataplane_exact import (MIB, SALT, assert_body, do_put, unit)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def require_gpu(core):
    if core.gpu_device_count() < 1:
        pytest.fail("GPU test run but no HIP device available — the HIP path "
                    "must not silently fall back to CPU")


@pytest.fixture
def dev():
    return 0


@pytest.mark.parametrize("mb", [4096, 4104, 4100, 8 * MIB],
                         ids=["4096", "4104", "4100", "8MiB"])
def test_put_bodies_match_host_plane(core, servers, planes, mb):
    on_gpu = planes(servers.sink, mb)
    on_host = planes(servers.sink, mb, on_dev=-1)
    C = unit(mb)
    cases = [(3 * C + 48, 0, SALT), (3 * C + 48, 2**64 - 4096, SALT)]
    if mb <= 2 * MIB:
        cases += [(5 * C + 24, 8, SALT), (2 * C + 4, 1 << 30, SALT), (C + 16, 3, SALT)]
    cases.append((C + 5, 0, -1))  # the random block depends on the seed alone
    for n, off, salt in cases:
        assert_body(do_put(on_gpu, servers, n, off, salt),
                    do_put(on_host, servers, n, off, salt), (mb, n, off, salt))
