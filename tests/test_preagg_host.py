"""Host-side checks of the hot-key pre-aggregation's control surface (no GPU)."""
import ctypes


def test_binding_exports_preagg_entry():
    import partitionedhashjoin_amd as phj
    from partitionedhashjoin_amd import _capi
    assert "phj_debug_preagg" in _capi.EXPORTED
    lib = _capi.load()   # loads on a GPU-less host; the prototypes are set, no compute call is made
    assert lib.phj_debug_preagg.argtypes[1] is ctypes.c_int and len(lib.phj_debug_preagg.argtypes) == 3
    assert (phj.PREAGG_AUTO, phj.PREAGG_OFF, phj.PREAGG_FORCED) == (0, 1, 2)
    assert lib.phj_debug_preagg(None, 0, None) == _capi.PHJ_ERR_INVALID   # a null context is refused before any device call
