"""The device's frame codec (stored Y, Cb, Cr frames with subsampled chroma <-> planar B, G, R; csrc/wm_pixel.hip
k_frame_codec) against its NumPy statement (tests/chroma_refs.py): bit-identical in both directions, for every
subsampling, through the host-pointer and the device-pointer entry points, on the 16-byte path and the byte-wise one."""
import ctypes as C

import numpy as np
import pytest

import chroma_refs as cr
import test_loop_trips as lt

pytestmark = pytest.mark.gpu

# (1, 1) .. (3, 5): odd edges in both axes; (16, 32), (32, 64): 16-byte path, more than one group per row; (17, 33), (18, 48):
# ragged tails / odd rows beside an aligned width; (64, 96): the video tests' frame
SHAPES = ((1, 1), (2, 2), (3, 5), (16, 32), (32, 64), (17, 33), (18, 48), (64, 96))


def _frames_inputs(n, H, W, sub, rng):
    fsz = cr.frame_bytes(H, W, sub)
    alt = rng.integers(0, 256, (n, fsz), dtype=np.uint8)
    alt[:, H * W:] = np.where(np.arange(fsz - H * W) % 2, 255, 0)           # chroma alternates 0 / 255 per sample
    return [rng.integers(0, 256, (n, fsz), dtype=np.uint8),                   # random bytes leave the BGR gamut: clipping
            np.zeros((n, fsz), np.uint8), np.full((n, fsz), 255, np.uint8), alt]


def _planes_inputs(n, H, W, sub, rng):
    return [rng.integers(0, 256, (n, 3, H, W), dtype=np.uint8), np.zeros((n, 3, H, W), np.uint8),
            np.full((n, 3, H, W), 255, np.uint8), cr.decode_frames(_frames_inputs(n, H, W, sub, rng)[3], H, W, sub)]


class _Dev:
    """device buffers for one call of a *_dev entry point; ``shift`` moves both bases off their 16-byte alignment"""

    def __init__(self, ctx, src: np.ndarray, out_bytes: int, shift: int = 0, fill: int = 0):
        self.ctx, self.shift, self.out_bytes = ctx, shift, out_bytes
        self.d_in = ctx.malloc(src.nbytes + 16 + shift); self.d_out = ctx.malloc(out_bytes + 16 + shift)
        ctx.h2d(self.d_in + shift, src)
        ctx.memset(self.d_out, fill, out_bytes + 16 + shift)

    def __enter__(self):
        return self.d_in + self.shift, self.d_out + self.shift

    def result(self) -> np.ndarray:
        out = np.empty(self.out_bytes, np.uint8)
        self.ctx.d2h(out, self.d_out + self.shift)
        self.ctx.sync()
        return out

    def __exit__(self, *exc):
        self.ctx.sync()
        self.ctx.free(self.d_in); self.ctx.free(self.d_out)


def _decode_dev(ctx, frames, H, W, sub, shift=0):
    n, fsz = frames.shape
    dev = _Dev(ctx, frames, n * 3 * H * W, shift)
    with dev as (d_f, d_p):
        ctx.yuv_frames_to_bgr_planes_u8_dev(d_f, d_p, n, H, W, sub, fsz)
        return dev.result().reshape(n, 3, H, W)


def _encode_dev(ctx, planes, sub, shift=0):
    n, _, H, W = planes.shape
    fsz = cr.frame_bytes(H, W, sub)
    dev = _Dev(ctx, planes, n * fsz, shift)
    with dev as (d_p, d_f):
        ctx.bgr_planes_to_yuv_frames_u8_dev(d_p, d_f, n, H, W, sub, fsz)
        return dev.result().reshape(n, fsz)


@pytest.mark.parametrize("sub", cr.SUBS, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("H,W", SHAPES)
def test_codec_equals_the_numpy_statement(gpu_ctx, H, W, sub):
    rng = np.random.default_rng(100 * H + W)
    for n in (1, 3):
        for k, frames in enumerate(_frames_inputs(n, H, W, sub, rng)):
            want = cr.decode_frames(frames, H, W, sub)
            got = gpu_ctx.yuv_frames_to_bgr_planes(frames, H, W, sub)
            assert got.shape == (n, 3, H, W) and np.array_equal(got, want), ("decode host", n, k)
            assert np.array_equal(_decode_dev(gpu_ctx, frames, H, W, sub), want), ("decode dev", n, k)
        for k, planes in enumerate(_planes_inputs(n, H, W, sub, rng)):
            want = cr.encode_frames(planes, sub)
            got = gpu_ctx.bgr_planes_to_yuv_frames(planes, sub)
            assert got.shape == want.shape and np.array_equal(got, want), ("encode host", n, k)
            assert np.array_equal(_encode_dev(gpu_ctx, planes, sub), want), ("encode dev", n, k)
    # bases off their alignment: the byte-wise path at a width the 16-byte path would take, same values
    frames = _frames_inputs(2, H, W, sub, rng)[0]
    assert np.array_equal(_decode_dev(gpu_ctx, frames, H, W, sub, shift=1), cr.decode_frames(frames, H, W, sub))
    planes = _planes_inputs(2, H, W, sub, rng)[0]
    assert np.array_equal(_encode_dev(gpu_ctx, planes, sub, shift=3), cr.encode_frames(planes, sub))


GUARD = 4096                       # bytes of 0xA5 the test puts behind a second-trip output, in the same allocation


def _second_trip_both_ways(ctx, frames, H, W, sub, what):
    """decode and encode through the *_dev entry points, bit-equal to chroma_refs, the guard behind each output untouched"""
    n, fsz = frames.shape
    assert fsz == cr.frame_bytes(H, W, sub)
    want = cr.decode_frames(frames, H, W, sub)
    planes = want if n > 1 else np.random.default_rng(W).integers(0, 256, (n, 3, H, W), dtype=np.uint8)
    enc = cr.encode_frames(planes, sub)
    for k in range(-2, 0) if n > 1 else ():                                # the second trip's frames: unlike every other, in and out
        for a in (frames, want.reshape(n, -1), enc):
            assert (a[k] != a).any(axis=1).sum() == n - 1
    dev = _Dev(ctx, frames, want.nbytes + GUARD, fill=0xA5)
    with dev as (d_f, d_p):
        ctx.yuv_frames_to_bgr_planes_u8_dev(d_f, d_p, n, H, W, sub, fsz)
        got = dev.result()
    bad = np.flatnonzero(got[:want.size] != want.reshape(-1))
    print(f"{what} decode: {bad.size} of {want.size} bytes differ (first {bad[:3].tolist()}, last {bad[-3:].tolist()})")
    assert bad.size == 0 and np.all(got[want.size:] == 0xA5)
    dev = _Dev(ctx, planes, enc.nbytes + GUARD, fill=0xA5)
    with dev as (d_p, d_f):
        ctx.bgr_planes_to_yuv_frames_u8_dev(d_p, d_f, n, H, W, sub, fsz)
        got = dev.result()
    bad = np.flatnonzero(got[:enc.size] != enc.reshape(-1))
    print(f"{what} encode: {bad.size} of {enc.size} bytes differ (first {bad[:3].tolist()}, last {bad[-3:].tolist()})")
    assert bad.size == 0 and np.all(got[enc.size:] == 0xA5)
    ctx.check_status()


@pytest.mark.parametrize("H,W,sub,vec", lt.CODEC_ITEM_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_codec_item_loop_second_trip(gpu_ctx, H, W, sub, vec):
    """k_frame_codec's item loop on grid_for's 2048 x 256 threads: one frame of more than 524 288 items (tests/test_loop_trips.py),
    on the byte-wise path (odd widths) at 4:4:4 and 4:2:0 and on the 16-byte path"""
    frames = np.random.default_rng(H).integers(0, 256, (1, cr.frame_bytes(H, W, sub)), dtype=np.uint8)
    _second_trip_both_ways(gpu_ctx, frames, H, W, sub, f"{H}x{W} {sub} {'16-byte' if vec else 'byte-wise'}")


@pytest.mark.parametrize("n,H,W,sub", lt.CODEC_FRAME_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_codec_frame_loop_second_trip(gpu_ctx, n, H, W, sub):
    """k_frame_codec's frame loop (fr += gridDim.y on at most 65 535 rows of workgroups): 65 537 frames of random bytes.  The
    last two - the second trip - differ from every other frame on both sides of both directions (asserted in the helper; the
    seeds are ones at which the 3-byte frames do), so a frame index that wrapped shows."""
    frames = np.random.default_rng(H).integers(0, 256, (n, cr.frame_bytes(H, W, sub)), dtype=np.uint8)
    assert n - 2 == lt.CODEC_FRAME_CAP
    _second_trip_both_ways(gpu_ctx, frames, H, W, sub, f"{n} frames of {H}x{W} {sub}")


@pytest.mark.parametrize("sub", cr.SUBS, ids=lambda s: "%dx%d" % s)
def test_chroma_survives_decode_then_encode(gpu_ctx, sub):
    """encode_chroma(replicate(c)) == c on the device too: an in-gamut frame comes back byte for byte"""
    H, W = 17, 48
    rng = np.random.default_rng(5)
    frames = rng.integers(96, 160, (2, cr.frame_bytes(H, W, sub)), dtype=np.uint8)
    planes = gpu_ctx.yuv_frames_to_bgr_planes(frames, H, W, sub)
    assert planes.min() > 0 and planes.max() < 255
    assert np.array_equal(gpu_ctx.bgr_planes_to_yuv_frames(planes, sub), frames)


@pytest.mark.parametrize("H,W,pad", [(16, 32, 48), (17, 33, 37), (32, 64, 5)])
def test_frame_stride_larger_than_a_frame(gpu_ctx, H, W, pad):
    """frames further apart than a frame: the bytes between them are not read on decode and not touched on encode"""
    sub, n = (2, 2), 3
    rng = np.random.default_rng(7)
    fsz = cr.frame_bytes(H, W, sub)
    buf = rng.integers(0, 256, (n, fsz + pad), dtype=np.uint8)
    want = cr.decode_frames(np.ascontiguousarray(buf[:, :fsz]), H, W, sub)
    assert np.array_equal(gpu_ctx.yuv_frames_to_bgr_planes(buf[:, :fsz], H, W, sub), want)
    planes = rng.integers(0, 256, (n, 3, H, W), dtype=np.uint8)
    enc = cr.encode_frames(planes, sub)
    out = np.full((n, fsz + pad), 0xA5, np.uint8)
    gpu_ctx.bgr_planes_to_yuv_frames(planes, sub, out=out[:, :fsz])
    assert np.array_equal(out[:, :fsz], enc) and np.all(out[:, fsz:] == 0xA5)
    # device pointers, the same stride
    dev = _Dev(gpu_ctx, buf, n * 3 * H * W)
    with dev as (d_f, d_p):
        gpu_ctx.yuv_frames_to_bgr_planes_u8_dev(d_f, d_p, n, H, W, sub, fsz + pad)
        assert np.array_equal(dev.result().reshape(n, 3, H, W), want)
    dev = _Dev(gpu_ctx, planes, n * (fsz + pad), fill=0xA5)
    with dev as (d_p, d_f):
        gpu_ctx.bgr_planes_to_yuv_frames_u8_dev(d_p, d_f, n, H, W, sub, fsz + pad)
        got = dev.result().reshape(n, fsz + pad)
    assert np.array_equal(got[:, :fsz], enc) and np.all(got[:, fsz:] == 0xA5)


@pytest.mark.parametrize("H,W", [(3, 5), (16, 32), (17, 33)])
def test_sub_1x1_equals_the_interleaved_colour_ops(gpu_ctx, H, W):
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (2, 3 * H * W), dtype=np.uint8)
    y, cb, crr = cr.split_frames(frames, H, W, (1, 1))
    planes = gpu_ctx.yuv_frames_to_bgr_planes(frames, H, W, (1, 1))
    for i in range(2):
        bgr = gpu_ctx.color("ycrcb2bgr", np.ascontiguousarray(np.stack([y[i], crr[i], cb[i]], axis=-1)))
        assert np.array_equal(np.moveaxis(planes[i], 0, -1), bgr)
    src = rng.integers(0, 256, (2, 3, H, W), dtype=np.uint8)
    enc = gpu_ctx.bgr_planes_to_yuv_frames(src, (1, 1))
    ey, ecb, ecr = cr.split_frames(enc, H, W, (1, 1))
    for i in range(2):
        ycc = gpu_ctx.color("bgr2ycrcb", np.ascontiguousarray(np.moveaxis(src[i], 0, -1)))
        assert np.array_equal(np.stack([ey[i], ecr[i], ecb[i]], axis=-1), ycc)


def test_empty_inputs_return_without_error(gpu_ctx):
    for sub in cr.SUBS:
        fsz = cr.frame_bytes(4, 6, sub)
        assert gpu_ctx.yuv_frames_to_bgr_planes(np.zeros((0, fsz), np.uint8), 4, 6, sub).shape == (0, 3, 4, 6)
        assert gpu_ctx.bgr_planes_to_yuv_frames(np.zeros((0, 3, 4, 6), np.uint8), sub).shape == (0, fsz)
        assert gpu_ctx.yuv_frames_to_bgr_planes(np.zeros((2, 0), np.uint8), 0, 6, sub).shape == (2, 3, 0, 6)
        assert gpu_ctx.bgr_planes_to_yuv_frames(np.zeros((2, 3, 4, 0), np.uint8), sub).shape == (2, 0)
        gpu_ctx.yuv_frames_to_bgr_planes_u8_dev(0, 0, 0, 4, 6, sub, fsz)          # nothing to do: the pointers are not looked at
        gpu_ctx.bgr_planes_to_yuv_frames_u8_dev(0, 0, 2, 0, 6, sub, 0)
    gpu_ctx.sync()


def test_bad_arguments_raise_with_their_message(gpu_ctx):
    H, W, sub = 4, 6, (2, 2)
    fsz = cr.frame_bytes(H, W, sub)
    frames = np.zeros((2, fsz), np.uint8); planes = np.zeros((2, 3, H, W), np.uint8)
    for bad in ((1, 2), (3, 1), (2, 3), (0, 0), (4, 4)):
        with pytest.raises(ValueError, match="subsampling"):
            gpu_ctx._call("wm_yuv_frames_to_bgr_planes_u8", frames.ctypes.data_as(C.c_void_p), planes.ctypes.data_as(C.c_void_p),
                          2, H, W, bad[0], bad[1], fsz)
        with pytest.raises(ValueError, match="subsampling"):
            gpu_ctx.bgr_planes_to_yuv_frames_u8_dev(0, 0, 0, H, W, bad, fsz)
    d = gpu_ctx.malloc(4096)
    try:
        for call in (gpu_ctx.yuv_frames_to_bgr_planes_u8_dev, gpu_ctx.bgr_planes_to_yuv_frames_u8_dev):
            with pytest.raises(ValueError, match="NULL"):
                call(0, d, 2, H, W, sub, fsz)
            with pytest.raises(ValueError, match="NULL"):
                call(d, 0, 2, H, W, sub, fsz)
            with pytest.raises(ValueError, match="frame_stride"):
                call(d, d + 2048, 2, H, W, sub, fsz - 1)
            with pytest.raises(ValueError, match="in place"):
                call(d, d, 2, H, W, sub, fsz)
            with pytest.raises(ValueError, match="in place"):
                call(d, d + fsz, 2, H, W, sub, fsz)                         # the second frame / plane reaches into the other side
            with pytest.raises(ValueError, match="negative"):
                call(d, d + 2048, -1, H, W, sub, fsz)
    finally:
        gpu_ctx.free(d)
    p = frames.ctypes.data_as(C.c_void_p)
    for name in ("wm_yuv_frames_to_bgr_planes_u8", "wm_bgr_planes_to_yuv_frames_u8"):
        with pytest.raises(ValueError, match="in place"):
            gpu_ctx._call(name, p, p, 1, H, W, 2, 2, fsz)
        with pytest.raises(ValueError, match="NULL"):
            gpu_ctx._call(name, p, None, 1, H, W, 2, 2, fsz)
        with pytest.raises(ValueError, match="frame_stride"):
            gpu_ctx._call(name, p, planes.ctypes.data_as(C.c_void_p), 2, H, W, 2, 2, fsz - 1)
    # the binding's own shape rules
    with pytest.raises(ValueError, match="frames must be"):
        gpu_ctx.yuv_frames_to_bgr_planes(np.zeros((2, fsz + 1), np.uint8), H, W, sub)
    with pytest.raises(ValueError, match="planes must be"):
        gpu_ctx.bgr_planes_to_yuv_frames(np.zeros((2, H, W), np.uint8), sub)
