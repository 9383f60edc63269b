"""What the -m gpu tests of the pack calls share: the api / ctx / oracle fixtures, images on the device and packs of them.

A new call's GPU test starts from these: `from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)` gives the module its own
Context (every fixture here has module scope, so the counters of the last call and the knobs a test sets are the module's own), a Batch
holds images and the oracle's streams of them, a Pack is a Batch encoded by the library, an OraclePack given pixels encoded by the oracle.
The guarded-output runners of the calls are in tests/gpu_calls.py, the 17.7 Mpx pack and its walk tables in tests/wide_cases.py.

No assert here is rewritten by pytest (this is no test module): every assert carries its operands in its message.  torch is imported
inside the functions that need it, so that the module can be imported without a GPU."""
import os

import numpy as np
import pytest

import resize_window as rw
from qoi_amd import tensors
from qoi_amd.resize import PLAIN

E_ARG = -1
GUARD = 0xA5
KINDS = ["noise", "constant", "photo", "uiflat", "sprite_alpha"]


@pytest.fixture(scope="module")
def api():
    import torch  # noqa: F401  (first, so the library binds to torch's HIP runtime)
    from qoi_amd import api as _api
    assert torch.cuda.is_available(), "torch sees no GPU"
    return _api


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle(ref, port):
    return ref or port


def dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


def filled(n, value=GUARD):
    import torch
    return torch.full((int(n),), value, dtype=torch.uint8, device="cuda")


def image(kind, w, h, ch, frame=0):
    from qoi_amd import synth
    if kind == "noise":
        return np.random.default_rng(w * 7919 + h * 31 + ch + frame).integers(0, 256, size=w * h * ch, dtype=np.uint8)
    return (synth.frame_rgba if ch == 4 else synth.frame_rgb)(kind, w, h, frame).reshape(-1)


class Batch:
    """Images on the device, tightly packed one behind the other, and the oracle's streams (computed once, never changed)."""

    def __init__(self, api, oracle, shapes, kinds):
        self.shapes = shapes
        self.px = [image(k, w, h, ch, frame=i) for i, ((w, h, ch), k) in enumerate(zip(shapes, kinds))]
        self.want = [oracle.encode(p, w, h, ch) for p, (w, h, ch) in zip(self.px, shapes)]
        self.lens = [len(s) for s in self.want]
        self.descs = [api.QoiDesc(w, h, ch, 0) for (w, h, ch) in shapes]
        self.bounds = [api.encode_bound(w, h, ch) for (w, h, ch) in shapes]
        self.pix_off = [int(x) for x in np.cumsum([0] + [p.size for p in self.px[:-1]])]
        self.d_px = dev(np.concatenate(self.px))
        self.n = len(shapes)


MIXED_SHAPES = [(1, 1, 4), (1, 97, 4), (131, 1, 3), (37, 23, 3), (257, 9, 4), (64, 48, 3), (333, 7, 4), (130, 70, 4)]


class Pack:
    """A batch encoded by the library into a pack (align 1), the pack's bytes on the host, and the oracle's decode of every stream as given
    (computed once per output channel count and size, never changed)."""

    def __init__(self, ctx, oracle, b):
        import torch
        cap = sum(b.bounds) + 256 * b.n
        self.b, self.oracle, self.n, self.shapes, self.descs = b, oracle, b.n, b.shapes, b.descs
        self.packed = filled(cap, 0)
        off = torch.zeros(b.n + 1, dtype=torch.int64, device="cuda")
        lens = torch.zeros(b.n, dtype=torch.int32, device="cuda")
        so, sizes = ctx.encode_images_packed(b.d_px.data_ptr(), b.pix_off, b.descs, 1, self.packed.data_ptr(), cap, off.data_ptr(), lens.data_ptr())
        self.so, self.sizes = [int(x) for x in so[:b.n]], [int(x) for x in sizes]
        self.host = self.packed.cpu().numpy().copy()
        self._decoded = {}

    def decoded(self, i, och, host=None, size=None):
        """the oracle's (lenient) decode of stream i as uint8[h, w, och]"""
        w, h, _ = self.shapes[i]
        if host is None and size is None:
            if (i, och) not in self._decoded:
                px, _ = self.oracle.decode(self.host[self.so[i]:self.so[i] + self.sizes[i]].tobytes(), och)
                self._decoded[(i, och)] = px.reshape(h, w, och)
            return self._decoded[(i, och)]
        host = self.host if host is None else host
        px, _ = self.oracle.decode(host[self.so[i]:self.so[i] + (self.sizes[i] if size is None else size)].tobytes(), och)
        assert px is not None, ("the oracle decodes nothing of stream", i, och, size)
        return px.reshape(h, w, och)


def batch_of(api, oracle, shapes, pixels):
    """a Batch of given pixels instead of a content class"""
    b = Batch.__new__(Batch)
    b.shapes, b.px, b.n = shapes, [np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in pixels], len(shapes)
    b.descs = [api.QoiDesc(w, h, ch, 0) for (w, h, ch) in shapes]
    b.bounds = [api.encode_bound(w, h, ch) for (w, h, ch) in shapes]
    b.pix_off = [int(x) for x in np.cumsum([0] + [p.size for p in b.px[:-1]])]
    b.d_px = dev(np.concatenate(b.px))
    return b


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


class OraclePack(Pack):
    """Given pixels as the oracle's streams, 3 bytes apart in one device buffer; decoded(): Pack's.  px[i]: the
    source pixels, window(): the sums of an item over the oracle's 4-channel decode, computed once per rectangle."""

    def __init__(self, api, oracle, shapes, pixels):
        self.oracle, self.n, self.shapes = oracle, len(shapes), shapes
        self.px = [np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in pixels]
        streams = [oracle.encode(p, w, h, ch) for p, (w, h, ch) in zip(self.px, shapes)]
        self.descs = [api.QoiDesc(w, h, ch, 0) for (w, h, ch) in shapes]
        self.sizes = [len(s) for s in streams]
        self.so = [int(x) for x in np.cumsum([5] + [n + 3 for n in self.sizes[:-1]])]
        self.host = np.zeros(self.so[-1] + self.sizes[-1] + 64, dtype=np.uint8)
        for o, s in zip(self.so, streams):
            self.host[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
        self.packed = dev(self.host)
        self._decoded, self._windows, self._boxes = {}, {}, {}

    def box(self, i, och, f, mode):
        """rw.box_thumbnail of image i, computed once"""
        key = (i, och, f, mode if och == 4 else PLAIN)
        if key not in self._boxes:
            self._boxes[key] = rw.box_thumbnail(self.decoded(i, och), f, mode).reshape(-1)
        return self._boxes[key]

    def window(self, it):
        key = tuple(it[:7])
        if key not in self._windows:
            self._windows[key] = rw.Window(self.decoded(it[0], 4), it[1:5], it[5:7])
        return self._windows[key]


IMAGENET = tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
SEGS = ["1024", "2048", "4096"]


@pytest.fixture(scope="module", params=SEGS)
def lctx(api, request):
    os.environ["QOIMI_SEG_BYTES"] = request.param
    os.environ["QOIMI_DEC_FUSED"] = "0"
    try:
        c = api.Context(0)
    finally:
        del os.environ["QOIMI_SEG_BYTES"]
        del os.environ["QOIMI_DEC_FUSED"]
    yield c
    c.close()


def packed_image(kind, w, h, ch, frame=0):
    from qoi_amd import synth
    if kind == "rand":
        return np.random.default_rng(w * 7919 + h * 31 + ch + frame).integers(0, 256, size=w * h * ch, dtype=np.uint8)
    return (synth.frame_rgba if ch == 4 else synth.frame_rgb)(kind, w, h, frame).reshape(-1)


class Item:
    def __init__(self, api, oracle, kind, w, h, ch, frame=0, stream=None):
        self.w, self.h, self.ch = w, h, ch
        self.stream = stream if stream is not None else oracle.encode(packed_image(kind, w, h, ch, frame), w, h, ch)
        self.desc = api.QoiDesc(w, h, ch, 0)
