"""CPU: gwd_conv_wgrad_takes_bias - which weight-gradient kernels also sum the bias gradient (gwd_conv_desc.dbias) - answered
through ctypes from the descriptor alone: no device is opened and nothing is launched."""
import ctypes

import pytest

from gw_depth_amd import hip

F32, BF16 = hip.F32, hip.BF16


@pytest.fixture(scope="module")
def takes():
    import os
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    lib.gwd_conv_wgrad_takes_bias.restype = ctypes.c_int
    lib.gwd_conv_wgrad_takes_bias.argtypes = [ctypes.POINTER(hip.ConvDesc), ctypes.c_int32]
    return lambda d, batched=0: lib.gwd_conv_wgrad_takes_bias(ctypes.byref(d), batched)


def desc(B, Hi, Wi, Cin, Cout, k=1, stride=1, dtype=BF16, zero_page=True, scale=False):
    """Weight-gradient descriptor of a k x k convolution with pad k // 2 (x = layer input, y = output gradient).  The pointers are
    16-byte aligned numbers that nobody dereferences."""
    d = hip.ConvDesc()
    d.x, d.y = 0x100000, 0x200000
    d.zero_page = 0x300000 if zero_page else None
    d.scale = 0x400000 if scale else None
    pad = k // 2
    d.B, d.Hi, d.Wi, d.Cin, d.Cout, d.KH, d.KW, d.stride, d.pad = B, Hi, Wi, Cin, Cout, k, k, stride, pad
    d.Ho, d.Wo = (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1
    d.gather, d.act_scale, d.dtype = hip.GATHER_CONV, 1.0, dtype
    return d


def test_descriptor_mirror_ends_with_dbias():
    assert hip.ConvDesc._fields_[-1][0] == "dbias" and hip.ConvDesc._fields_[-2][0] == "reserved"
    assert ctypes.sizeof(hip.ConvDesc) == 184 and hip.ConvDesc.dbias.offset == 176


@pytest.mark.parametrize("batched", [0, 1])
def test_linear_takes_bias(takes, batched):
    assert takes(desc(1031, 1, 1, 320, 200), batched) == 1
    assert takes(desc(153600, 1, 1, 64, 256), batched) == 1


@pytest.mark.parametrize("stride", [1, 2])
def test_conv3x3_on_the_dma_family_takes_bias(takes, stride):
    assert takes(desc(8, 60, 80, 256, 256, k=3, stride=stride)) == 1
    assert takes(desc(8, 60, 80, 256, 256, k=3, stride=stride), 1) == 1
    assert takes(desc(2, 13, 17, 16, 72, k=3, stride=stride)) == 1


def test_fp32_declines(takes):
    assert takes(desc(1031, 1, 1, 320, 200, dtype=F32)) == 0
    assert takes(desc(8, 60, 80, 256, 256, k=3, dtype=F32), 1) == 0


def test_no_zero_page_declines(takes):
    assert takes(desc(1031, 1, 1, 320, 200, zero_page=False)) == 0          # the register-staged igemm_wgrad_kernel


def test_scale_declines(takes):
    assert takes(desc(1031, 1, 1, 320, 200, scale=True)) == 0
    assert takes(desc(8, 60, 80, 256, 256, k=3, scale=True), 1) == 0


def test_wgrad_taps_shape_declines(takes):
    assert takes(desc(8, 120, 160, 160, 160, k=3)) == 0
    assert takes(desc(8, 120, 160, 160, 160, k=3), 1) == 0


def test_tile_conv_shape_64_to_64_declines(takes):
    assert takes(desc(8, 240, 320, 64, 64, k=3)) == 0
    assert takes(desc(8, 240, 320, 64, 64, k=3), 1) == 0


@pytest.mark.parametrize("cin,cout,hw", [(64, 32, (240, 320)), (32, 32, (240, 320)), (32, 32, (480, 640)), (32, 64, (240, 320))])
def test_tile_conv_family_declines(takes, cin, cout, hw):
    """3x3 / stride 1 over 32- / 64-channel maps of >= 131072 pixels: tconv_wgrad_kernel takes the members with 32 output-gradient
    channels, the others run on the generic kernels; the query declines the family as a whole (csrc/tileconv.hip)."""
    assert takes(desc(8, hw[0], hw[1], cin, cout, k=3)) == 0
    assert takes(desc(8, hw[0], hw[1], cin, cout, k=3), 1) == 0


def test_tile_conv_channels_on_a_small_map_take_bias(takes):
    assert takes(desc(8, 60, 80, 64, 64, k=3)) == 1                        # 38 400 pixels: not a tile-conv layer


@pytest.mark.parametrize("cout", [1, 2])
def test_thin_head_declines(takes, cout):
    assert takes(desc(8, 480, 640, 32, cout, k=3)) == 0
    assert takes(desc(8, 480, 640, 32, cout, k=3), 1) == 0


def test_bad_descriptor_declines(takes):
    d = desc(1031, 1, 1, 320, 200)
    d.x = None
    assert takes(d) == 0
