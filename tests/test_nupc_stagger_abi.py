"""CPU: the staggered-switch calls of include/bfhip_nupc.h are exported, bound on Nupc, and fail
cleanly on a NULL handle (no HIP call is made)."""
import brutefir_amd as bf

EINVAL, ESTATE = -1, -5


def test_symbols_exported_and_bound():
    L = bf.lib()
    for name in ("bfhip_nupc_set_switch_mode", "bfhip_nupc_get_switch_mode", "bfhip_nupc_switch_frame_segment"):
        assert hasattr(L, name), name
    for name in ("set_switch_mode", "switch_mode", "switch_frame_segment"):
        assert callable(getattr(bf.Nupc, name)), name
    assert (bf.SWITCH_ALIGNED, bf.SWITCH_STAGGERED) == (0, 1)


def test_null_handle():
    L = bf.lib()
    assert L.bfhip_nupc_set_switch_mode(None, bf.SWITCH_STAGGERED) == EINVAL
    assert L.bfhip_nupc_get_switch_mode(None) < 0
    # -1 means "no switch yet": a bad handle must not look like it
    assert L.bfhip_nupc_switch_frame_segment(None, 0) < -1
    assert L.bfhip_nupc_switch_frame_segment(None, 0) == ESTATE
    assert L.bfhip_nupc_last_error()
