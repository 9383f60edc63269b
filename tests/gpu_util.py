"""Helpers for the -m gpu tests: device buffers via torch (plumbing only)."""
import ctypes

import numpy as np


def torch_mod():
    import torch
    return torch


class DeviceBatch:
    """Owns device buffers for an encode/decode batch of equally shaped images."""

    def __init__(self, ctx, width, height, channels, n):
        torch = torch_mod()
        from qoi_amd import api
        self.ctx, self.w, self.h, self.ch, self.n = ctx, width, height, channels, n
        self.npx = width * height
        self.desc = api.QoiDesc(width, height, channels, 0)
        self.pixel_stride = (self.npx * channels + 255) // 256 * 256
        self.stream_stride = (api.encode_bound(width, height, channels) + 255) // 256 * 256
        self.pixels = torch.zeros(n * self.pixel_stride, dtype=torch.uint8, device="cuda")
        self.streams = torch.zeros(n * self.stream_stride, dtype=torch.uint8, device="cuda")
        self.lens = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream

    def upload(self, i, arr):
        torch = torch_mod()
        a = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1))
        self.pixels[i * self.pixel_stride:i * self.pixel_stride + a.numel()].copy_(a)

    def encode(self):
        self.ctx.encode_batch(self.pixels.data_ptr(), self.pixel_stride, self.desc, self.n,
                              self.streams.data_ptr(), self.stream_stride, self.lens.data_ptr(), self.stream)
        self.ctx.encode_status(self.stream)
        return self.lens.cpu().numpy()

    def stream_bytes(self, i, length):
        return self.streams[i * self.stream_stride:i * self.stream_stride + int(length)].cpu().numpy().tobytes()

    def decode_into(self, out, lens, out_channels=0):
        """Decode this batch's streams into torch uint8 buffer `out` (pixel_stride spacing)."""
        och = out_channels or self.ch
        stride = (self.npx * och + 255) // 256 * 256
        self.ctx.decode_batch(self.streams.data_ptr(), self.stream_stride, [int(x) for x in lens],
                              [self.desc] * self.n, out_channels, out.data_ptr(), stride, self.stream)
        return stride


GUARD = 64                # bytes in front of a base and behind a buffer's last slot that no call may touch (a multiple of 16)
STREAM_FILL = 0xEE
OUT_FILL = 0xCD


class GuardedRegion:
    """A buffer of `size` bytes pre-filled with `fill` in which slot i begins at byte starts[i] - the arithmetic of "what may be
    written, everything else is still the fill byte", on a host copy of the whole buffer (numpy only: tested without a GPU)."""

    def __init__(self, size, starts, fill):
        self.size, self.starts, self.fill = int(size), [int(s) for s in starts], int(fill)

    @classmethod
    def strided(cls, front, stride, n, fill, tail=GUARD):
        return cls(front + n * stride + tail, [front + i * stride for i in range(n)], fill)

    def writable(self, lengths):
        """bool[size]: True on the first lengths[i] bytes of every slot"""
        assert len(lengths) == len(self.starts)
        m = np.zeros(self.size, dtype=bool)
        for s, k in zip(self.starts, lengths):
            assert 0 <= s and s + int(k) <= self.size, (s, int(k), self.size)
            m[s:s + int(k)] = True
        return m

    def where(self, k, lengths):
        """words for byte k of the buffer: which slot's writable bytes lie in front of it, and how far"""
        at = [(s + int(n), i) for i, (s, n) in enumerate(zip(self.starts, lengths)) if s + int(n) <= k]
        if not at:
            return f"{min(self.starts) - k} bytes in front of the first slot"
        end, i = max(at)
        return f"{k - end} bytes behind the {int(lengths[i])} writable bytes of slot {i}"

    def assert_untouched(self, host, lengths, what):
        """Every byte of `host` (the whole buffer) outside the first lengths[i] bytes of the slots still holds the fill byte."""
        host = np.asarray(host)
        assert host.dtype == np.uint8 and host.size == self.size, (host.dtype, host.size, self.size)
        bad = np.flatnonzero(~self.writable(lengths) & (host != self.fill))
        if bad.size:
            k = int(bad[0])
            raise AssertionError(f"{what}: {bad.size} bytes written outside their range, the first at byte {k} of the buffer "
                                 f"({self.where(k, lengths)}): {int(host[k]):#04x}, not {self.fill:#04x}")


class EdgeBatch:
    """DeviceBatch for what the C-ABI leaves to the caller and DeviceBatch never does: bases at odd addresses (po, so, oo in 1..15
    bytes behind a 16-byte boundary), pixel_stride = npx*ch + dp and stream_stride = bound + ds with dp, ds down to 0, the stream
    buffer pre-filled with 0xEE, a decode output with 0xCD, GUARD bytes in front of every base and behind every buffer's last slot.
    encode() / decode() return the WHOLE buffer as a host array; the check_* methods compare it with the expected bytes and the fill.
    ctx None: the layout and the checks alone, on host arrays (no device buffers)."""

    def __init__(self, ctx, width, height, channels, n, po=1, so=1, oo=1, dp=0, ds=0):
        from qoi_amd import api
        assert all(1 <= o <= 15 for o in (po, so, oo)) and dp >= 0 and ds >= 0
        self.ctx, self.w, self.h, self.ch, self.n = ctx, width, height, channels, n
        self.po, self.so, self.oo = po, so, oo
        self.npx = width * height
        self.desc = api.QoiDesc(width, height, channels, 0)
        self.bound = api.encode_bound(width, height, channels)
        self.pixel_stride = self.npx * channels + dp
        self.stream_stride = self.bound + ds
        self.preg = GuardedRegion.strided(GUARD + po, self.pixel_stride, n, 0)
        self.sreg = GuardedRegion.strided(GUARD + so, self.stream_stride, n, STREAM_FILL)
        if ctx is None:
            return
        torch = torch_mod()
        self.pixels = torch.zeros(self.preg.size, dtype=torch.uint8, device="cuda")
        self.streams = torch.full((self.sreg.size,), STREAM_FILL, dtype=torch.uint8, device="cuda")
        self.lens = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream
        assert self.pixels.data_ptr() % 16 == 0 and self.streams.data_ptr() % 16 == 0
        self.d_pixels = self.pixels.data_ptr() + GUARD + po
        self.d_streams = self.streams.data_ptr() + GUARD + so

    def stream_address_residues(self):
        """(address of stream i) & 15 for every image, given a 16-byte aligned allocation"""
        return [(self.so + i * self.stream_stride) & 15 for i in range(self.n)]

    def upload(self, i, arr):
        torch = torch_mod()
        a = torch.from_numpy(np.array(arr, dtype=np.uint8).reshape(-1))            # (a copy: the source may be read-only)
        assert a.numel() == self.npx * self.ch
        self.pixels[self.preg.starts[i]:self.preg.starts[i] + a.numel()].copy_(a)

    def encode(self):
        """encode_batch + encode_status -> (lengths, host copy of the whole stream buffer)"""
        self.ctx.encode_batch(self.d_pixels, self.pixel_stride, self.desc, self.n, self.d_streams, self.stream_stride, self.lens.data_ptr(), self.stream)
        self.ctx.encode_status(self.stream)
        return self.lens.cpu().numpy(), self.streams.cpu().numpy()

    def check_streams(self, host, lens, want, what):
        """Lengths and bytes equal `want` (the reference's streams); no byte outside the slots' `bound` bytes was written (the
        contract of the header), nor any between a stream's end and its slot's bound (what tests/fuzz_encode.py --odd-strides holds
        the library to)."""
        assert [int(x) for x in lens] == [len(s) for s in want], (what, [int(x) for x in lens], [len(s) for s in want])
        for i, s in enumerate(want):
            got = host[self.sreg.starts[i]:self.sreg.starts[i] + len(s)]
            if got.tobytes() != s:
                k = int(np.argmax(got != np.frombuffer(s, dtype=np.uint8)))
                raise AssertionError(f"{what}: stream {i} differs from the reference's at byte {k} of {len(s)}")
        self.sreg.assert_untouched(host, [self.bound] * self.n, f"{what}: outside the slots")
        self.sreg.assert_untouched(host, [len(s) for s in want], f"{what}: behind a stream")

    def decode(self, lens, out_channels):
        """qoimi_decode_batch from the odd stream base into an odd output base, pixel_stride == npx*och exactly ->
        (host copy of the whole output buffer, its GuardedRegion)"""
        torch = torch_mod()
        och = out_channels or self.ch
        region = GuardedRegion.strided(GUARD + self.oo, self.npx * och, self.n, OUT_FILL)
        out = torch.full((region.size,), OUT_FILL, dtype=torch.uint8, device="cuda")
        assert out.data_ptr() % 16 == 0
        self.ctx.decode_batch(self.d_streams, self.stream_stride, [int(x) for x in lens], [self.desc] * self.n, out_channels,
                              out.data_ptr() + GUARD + self.oo, self.npx * och, self.stream)
        return out.cpu().numpy(), region

    def check_pixels(self, host, region, want, what):
        """Every image equals want[i] (flat uint8) and nothing around the images was written."""
        for i, px in enumerate(want):
            got = host[region.starts[i]:region.starts[i] + px.size]
            if not np.array_equal(got, px.reshape(-1)):
                raise AssertionError(f"{what}: image {i} differs from the reference decoder's at byte {int(np.argmax(got != px.reshape(-1)))}")
        region.assert_untouched(host, [px.size for px in want], f"{what}: around the images")
