"""Host side of the streaming stride-2 data-gradient kernel (csrc/conv_s2dgrad.hip): the eligibility probe on both sides of every
bound of its rule, the A/B switch, and the planner's launch counts, which the new kernel leaves as they were.  No GPU."""
import ctypes as C

from downgan_amd import _lib


def geom(**kw):
    return _lib.ConvGeom(**dict(dict(dtype=_lib.DG_BF16, N=2, H=64, W=64, Cin=128, Cout=128, stride=2, cin_real=0,
                                     pixel_shuffle=0, ldx=128, ldy=128), **kw))


def probe(g, ep=None):
    return _lib.lib().dg_conv3x3_dgrad_stream_eligible(C.byref(g), C.byref(ep) if ep is not None else None)


def test_geometry_bounds_of_the_rule():
    assert probe(geom()) == 1
    assert probe(geom(N=32, H=1024, W=1024)) == 1                  # the critic's features.2 at the benchmarked batch
    assert probe(geom(H=2, W=2)) == 1                              # one dy pixel
    assert probe(geom(dtype=_lib.DG_F32)) == 0
    assert probe(geom(stride=1)) == 0
    for c in (64, 256):
        assert probe(geom(Cin=c, ldx=c)) == 0, c
        assert probe(geom(Cout=c, ldy=c)) == 0, c
    assert probe(geom(ldx=256)) == 0                               # a channel slice of a wider dx
    assert probe(geom(ldy=256)) == 0                               # ... of a wider dy
    # row-step limit of the halo kernel (gg_halo_row_step_ok): W/2 * 128 channels * 2 bytes < 8 MiB
    assert probe(geom(H=2, W=65534)) == 1
    assert probe(geom(H=2, W=65536)) == 0
    # one image of dx below 2 GiB: H * W * 256 bytes < 2^31
    assert probe(geom(H=2048, W=4094)) == 1
    assert probe(geom(H=2048, W=4096)) == 0
    # geometries the planner refuses keep their status
    assert probe(geom(H=63)) < 0
    assert probe(geom(stride=3)) < 0


def test_epilogue_bounds_of_the_rule():
    word = C.c_uint16(0)
    p = C.addressof(word)                                # any non-null address: the probe never reads through it
    assert probe(geom(), _lib.Epilogue()) == 1
    assert probe(geom(), _lib.Epilogue(mask_slope=0.2)) == 1
    assert probe(geom(), _lib.Epilogue(mask_bits=p, mask_slope=0.2)) == 1
    ptr_fields = ("bias", "r1", "r2", "mask", "out_bits", "out_q", "out_qs", "out_u", "out_ue", "out_amax")
    for f in ptr_fields:
        assert probe(geom(), _lib.Epilogue(**{f: p})) == 0, f
        assert probe(geom(), _lib.Epilogue(**{f: p, "mask_bits": p})) == 0, f
    for f in ("has_act", "accumulate", "mask_last", "skip_y"):
        assert probe(geom(), _lib.Epilogue(**{f: 1})) == 0, f
    assert probe(geom(), _lib.Epilogue(mask_c0=64)) == 0
    fields = {f[0] for f in _lib.Epilogue._fields_}
    covered = set(ptr_fields) | {"has_act", "accumulate", "mask_last", "skip_y", "mask_c0", "mask_bits", "mask_slope"}
    # scalars that only qualify an operand the rule already refuses
    assert fields - covered <= {"act_slope", "ldr1", "s1", "ldr2", "s2", "ldmask", "ldqs"}, fields - covered


def test_switch_returns_the_previous_value_and_defaults_to_on():
    lib = _lib.lib()
    assert lib.dg_set_s2_dgrad_stream(0) == 1
    try:
        assert lib.dg_set_s2_dgrad_stream(4) == 0
        assert lib.dg_set_s2_dgrad_stream(-3) == 4
        assert lib.dg_set_s2_dgrad_stream(1) == 0
        assert probe(geom()) == 1                                  # the probe answers for the rule, not for the switch
    finally:
        lib.dg_set_s2_dgrad_stream(1)


def test_planner_launch_counts_are_unchanged():
    lib = _lib.lib()
    assert lib.dg_conv3x3_dgrad_launches(C.byref(geom())) == 1
    assert lib.dg_conv3x3_dgrad_launches(C.byref(geom(stride=1))) == 1
    assert lib.dg_conv3x3_dgrad_launches(C.byref(geom(Cin=16, ldx=16))) == 4
    assert lib.dg_conv3x3_dgrad_launches(C.byref(geom(W=8190, Cout=1024, ldy=1024))) == 1
    assert lib.dg_conv3x3_dgrad_launches(C.byref(geom(W=8192, Cout=1024, ldy=1024))) == 4
    assert lib.dg_conv3x3_dgrad_launches(C.byref(geom(dtype=_lib.DG_F32, W=4096, Cout=1024, ldy=1024))) == 4
    assert lib.dg_conv3x3_dgrad_launches(C.byref(geom(H=2, W=65536))) == 4      # beyond the row step: no merged launch either
