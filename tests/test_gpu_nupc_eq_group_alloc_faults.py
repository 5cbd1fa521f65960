"""GPU: every allocation that bfhip_nupc_reserve_eq_group adds fails cleanly.  A life is create .. finalize of
a 2x2 crossbar with bases on two filters; bfhip_selftest_fail_alloc counts its device and pinned allocations.
The reservation's allocations (a result per member beyond the first, and the pinned non-finite words) come
behind every allocation of the life without it: with each of them failing in turn finalize answers
BFHIP_ENOMEM, destroy is clean, and a life afterwards works; without the reservation the life makes the
allocations it made before, and the first of the new ones is never reached."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ENOMEM = -3
GROUP = 4
FAR = 1 << 20


def _life(hip, group, arm=0):
    """-> (allocations made, finalize's error or None)"""
    nu = hip.Nupc([16, 32, 64], [2, 2, 4], 4, 2, 2)
    err = None
    try:
        nu.reserve_update()
        nu.reserve_eq(256)
        nu.reserve_eq_minimum()
        if group:
            nu.reserve_eq_group(group)
        rng = np.random.default_rng(3)
        for f in range(4):
            nu.add_filter(f // 2, f % 2, (rng.standard_normal(352) / 20).astype(np.float32))
            assert nu.add_coeff(f, (rng.standard_normal(352) / 20).astype(np.float32)) == 1
        nu.reserve_eq_base(0)
        nu.reserve_eq_base(2)
        hip.lib().bfhip_selftest_fail_alloc(arm or FAR)
        r = hip.lib().bfhip_nupc_finalize(nu.h)
        if r < 0:
            err = (r, hip.lib().bfhip_nupc_last_error())
    finally:
        left = hip.lib().bfhip_selftest_fail_alloc(0)
        nu.close()
    return (arm or FAR) - left, err


def test_every_allocation_of_the_group_reservation_fails_cleanly(hip):
    _life(hip, 0)                                               # warm-up: module loads, runtime pools
    plain, err = _life(hip, 0)
    assert err is None and plain > 20
    with_group, err = _life(hip, GROUP)
    assert err is None
    # three more results (two filters have bases: the slots exist) and one pinned array of words
    assert with_group == plain + (GROUP - 1) + 1
    for k in range(plain + 1, with_group + 1):
        made, err = _life(hip, GROUP, arm=k)
        assert made == k and err is not None and err[0] == ENOMEM, (k, made, err)
        assert b"reserve_eq_group" in err[1]
        assert _life(hip, 0, arm=k) == (plain, None)            # without the reservation it is never reached
    assert _life(hip, GROUP, arm=with_group + 1) == (with_group, None)
    assert _life(hip, GROUP) == (with_group, None) and _life(hip, 0) == (plain, None)


def test_a_finalized_group_convolver_works_after_the_faults(hip):
    nu = hip.Nupc([16, 32, 64], [2, 2, 4], 4, 1, 2)
    nu.reserve_update()
    nu.reserve_eq(256)
    nu.reserve_eq_group(2)
    h = (np.random.default_rng(4).standard_normal(352) / 20).astype(np.float32)
    for f in range(2):
        nu.add_filter(0, f, h)
        assert nu.add_coeff(f, h[::-1].copy()) == 1
    nu.finalize()
    nu.render_eq_group_async([0, 1], [1, 1], None, 256, [0.0, 0.5], [1.0, 2.0], [0.0, 0.0])
    assert nu.update_wait() == 0 and nu.update_result_member(1) == 0
    nu.close()
