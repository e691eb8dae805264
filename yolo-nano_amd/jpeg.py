"""Baseline JPEG files -> uint8 [h,w,3] BGR frames on the device, byte for byte what cv2.imread returns (yn_jpeg_*).

    frame = imread("000001.jpg")                       # the stand-in for cv2.imread in data/voc.py:pull_image and data/coco.py
    frames = JPEGDecoder(max_batch=32).batch(blobs)    # blobs: bytes objects; one upload and two kernel launches per 32 files

The Huffman stage runs on the host, threaded over the files of a batch; dequantisation, the inverse DCT, chroma upsampling and the colour
conversion run on the device.  The frames go straight into ValTransforms.batch / TrainTransforms.batch / Mosaic.batch / evaluate /
Visualizer.batch, which take CUDA uint8 frames as they are.  Files outside the baseline subset (progressive, arithmetic, 12-bit, CMYK,
unusual sampling factors) are refused with a reason; there is no host decoder to fall back to.  `info` and `coefficients` need no GPU.

    JPEGDecoder(max_batch=32, entropy="device")        # opt-in (yn_jpeg_entropy): the device decodes the Huffman stage too

With entropy="device" the host only parses the markers and copies each scan once; frames, statuses and reasons stay those of the default
in every case (a file the device cannot vouch for is decoded by the host after all), and a batch() call waits for one result word per file.
`scan_prepare` (that copy pass alone) needs no GPU.

    imwrite("000001.jpg", frame)                        # the stand-in for cv2.imwrite in test.py / demo.py (yn_jpeg_enc_*)
    files = JPEGEncoder(max_batch=32).batch(frames)     # bytes objects: the whole encoder runs on the device, the files come down

`quant_tables` and `header` need no GPU."""
import ctypes
import os

import numpy as np

from . import capi

OK, UNSUPPORTED, CORRUPT, TOO_LARGE = 0, 1, 2, 3
STATUS_NAMES = {OK: "ok", UNSUPPORTED: "unsupported", CORRUPT: "corrupt", TOO_LARGE: "too large"}


def _buffer(blob):
    """bytes-like -> (object that keeps the memory alive, address, length)."""
    a = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
    return a, a.ctypes.data, int(a.size)


def info(blob):
    """Header fields of one file (yn_jpeg_info; host only): dict(w, h, components, h_samp, v_samp, restart_interval, sof, status, reason)."""
    lib = capi.load_library()
    keep, ptr, n = _buffer(blob)
    out = np.zeros(8, dtype=np.int32)
    st = lib.yn_jpeg_info(ptr, n, out.ctypes.data)
    return dict(w=int(out[0]), h=int(out[1]), components=int(out[2]), h_samp=int(out[3]), v_samp=int(out[4]), restart_interval=int(out[5]),
                sof=int(out[6]), status=int(st), reason=lib.yn_jpeg_reason(None, 0).decode() if st else "")


def coefficient_count(meta):
    """int16 elements yn_jpeg_coefficients writes for a file with these header fields (the MCU-padded block grids, 64 per block)."""
    mw = -(-meta["w"] // (8 * meta["h_samp"]))
    mh = -(-meta["h"] // (8 * meta["v_samp"]))
    blocks = mw * mh * (meta["h_samp"] * meta["v_samp"] + (2 if meta["components"] == 3 else 0))
    return 64 * blocks


def coefficients(blob):
    """The entropy stage alone (yn_jpeg_coefficients; host only) -> dict(status, reason, coef = [int16 [bh, bw, 64] per component],
    qt uint16 [3, 64] natural order, grid int32 [3, 2])."""
    lib = capi.load_library()
    meta = info(blob)
    if meta["status"]:
        return dict(status=meta["status"], reason=meta["reason"], coef=[], qt=None, grid=None)
    keep, ptr, n = _buffer(blob)
    cap = coefficient_count(meta)
    flat = np.zeros(cap, dtype=np.int16)
    qt = np.zeros((3, 64), dtype=np.uint16)
    grid = np.zeros((3, 2), dtype=np.int32)
    st = ctypes.c_int()
    lib.yn_jpeg_coefficients(ptr, n, flat.ctypes.data, cap, qt.ctypes.data, grid.ctypes.data, ctypes.byref(st))
    coef, off = [], 0
    for c in range(meta["components"]):
        k = int(grid[c, 0]) * int(grid[c, 1]) * 64
        coef.append(flat[off:off + k].reshape(int(grid[c, 0]), int(grid[c, 1]), 64))
        off += k
    return dict(status=int(st.value), reason=lib.yn_jpeg_reason(None, 0).decode() if st.value else "", coef=coef, qt=qt, grid=grid)


def scan_prepare(blob):
    """The copy pass of the device entropy mode alone (yn_jpeg_scan_prepare; host only) -> dict(status, reason, scan = the entropy-coded
    data without byte stuffing and restart markers (bytes), segments int32 [n, 2] = first byte and first MCU of every restart segment,
    host = True when the file must take the host decoder, expected = the segments its header asks for)."""
    lib = capi.load_library()
    keep, ptr, n = _buffer(blob)
    info4 = np.zeros(4, dtype=np.int32)
    st = lib.yn_jpeg_scan_prepare(ptr, n, None, 0, None, 0, info4.ctypes.data)                # asks for the segment count
    if st != TOO_LARGE:
        return dict(status=int(st), reason=lib.yn_jpeg_reason(None, 0).decode() if st else "", scan=b"", segments=np.zeros((0, 2), np.int32), host=True, expected=0)
    out = np.zeros(max(n, 1), dtype=np.uint8)
    segs = np.zeros((max(int(info4[3]), 1), 2), dtype=np.int32)
    st = lib.yn_jpeg_scan_prepare(ptr, n, out.ctypes.data, out.size, segs.ctypes.data, segs.shape[0], info4.ctypes.data)
    return dict(status=int(st), reason=lib.yn_jpeg_reason(None, 0).decode() if st else "", scan=out[:int(info4[0])].tobytes(),
                segments=segs[:int(info4[1])].copy(), host=bool(info4[2]), expected=int(info4[3]))


ENTROPY_MODES = {"host": 0, "device": 1}


class JPEGDecoder(object):
    """A yn_jpeg object: two pinned staging slots, so the host decodes one chunk while the previous one uploads and runs.
    threads=None: min(16, $OMP_NUM_THREADS or 8) host workers.  Staging grows by itself (the object is recreated).
    entropy="device": the Huffman stage runs on the device in subsequences of subseq_bits (a multiple of 32) that synchronise in at most
    max_rounds rounds (None: the library's defaults); the results are those of entropy="host", the default, in every case."""

    def __init__(self, max_batch=32, threads=None, handle=None, device=None, staging_bytes=None, entropy="host", subseq_bits=None, max_rounds=None):
        if entropy not in ENTROPY_MODES:
            raise ValueError("entropy %r is not one of %s" % (entropy, ", ".join(sorted(ENTROPY_MODES))))
        self.entropy, self.subseq_bits, self.max_rounds = entropy, subseq_bits, max_rounds
        self.lib = capi.load_library()
        self.max_batch = int(max_batch)
        self.threads = int(threads) if threads is not None else min(16, int(os.environ.get("OMP_NUM_THREADS", 8)))
        self._handle, self._device = handle, device
        self.j = None
        self.staging_bytes = 0
        self._create(int(staging_bytes) if staging_bytes else self.max_batch * 640 * 480 * 3)       # 4:2:0 VGA frames to begin with

    def _h(self, handle=None):
        if handle is not None:
            return handle
        if self._handle is None:                               # a bare handle: only its stream / error plumbing is used
            import torch
            from . import arch
            dev = self._device if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            self._handle = capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x", device=dev)
        return self._handle

    def _create(self, staging_bytes):
        h = self._h()
        self.close()
        j = ctypes.c_void_p()
        h._ck(self.lib.yn_jpeg_create(h.h, self.max_batch, int(staging_bytes), self.threads, ctypes.byref(j)), "yn_jpeg_create")
        self.j, self.staging_bytes = j, int(staging_bytes)
        if self.entropy != "host" or self.subseq_bits is not None or self.max_rounds is not None:
            if self.lib.yn_jpeg_entropy(j, ENTROPY_MODES[self.entropy], int(self.subseq_bits or 0), int(self.max_rounds or 0)):
                reason = self.lib.yn_jpeg_reason(None, 0).decode()
                self.close()
                raise ValueError(reason)

    def entropy_stats(self):
        """{'device_files', 'host_files'} since the object was (re)created, {'rounds_last', 'subseqs_last'} of the last chunk
        (yn_jpeg_entropy_stats); all 0 with entropy="host"."""
        d, hf = ctypes.c_int64(), ctypes.c_int64()
        r, n = ctypes.c_int32(), ctypes.c_int32()
        self.lib.yn_jpeg_entropy_stats(self.j, ctypes.byref(d), ctypes.byref(hf), ctypes.byref(r), ctypes.byref(n))
        return {"device_files": int(d.value), "host_files": int(hf.value), "rounds_last": int(r.value), "subseqs_last": int(n.value)}

    def entropy_timing(self, handle=None):
        """Of the last chunk decoded with entropy="device" (yn_jpeg_entropy_timing; synchronises): milliseconds of the upload of scans and
        tables, the clearing, and the four entropy kernels, and 'decodes_per_subseq' of the synchronisation (1 = a serial decoder's work)."""
        h = self._h(handle)
        ms = (ctypes.c_float * 7)()
        h._ck(self.lib.yn_jpeg_entropy_timing(h.h, self.j, ctypes.cast(ms, ctypes.c_void_p)), "yn_jpeg_entropy_timing")
        return dict(zip(("upload_ms", "clear_ms", "first_ms", "sync_ms", "write_ms", "dc_ms", "decodes_per_subseq"), [float(v) for v in ms]))

    def device_coefficients(self, i, meta, handle=None):
        """The coefficients of file i of the last chunk as the device's entropy stage left them (yn_jpeg_device_coefficients), as
        `coefficients` returns a file's; meta = info(file)."""
        h = self._h(handle)
        flat = np.zeros(coefficient_count(meta), dtype=np.int16)
        h._ck(self.lib.yn_jpeg_device_coefficients(h.h, self.j, int(i), flat.ctypes.data, flat.size), "yn_jpeg_device_coefficients")
        mw, mh = -(-meta["w"] // (8 * meta["h_samp"])), -(-meta["h"] // (8 * meta["v_samp"]))
        grids = [(mh * meta["v_samp"], mw * meta["h_samp"])] + [(mh, mw)] * (meta["components"] - 1)
        out, off = [], 0
        for a, b in grids:
            out.append(flat[off:off + 64 * a * b].reshape(a, b, 64))
            off += 64 * a * b
        return out

    def entropy_states(self, i, handle=None):
        """int32 [subsequences, 4] of file i of the last chunk (yn_jpeg_entropy_states): bit, unit in the MCU, zigzag index, blocks before."""
        h = self._h(handle)
        out = np.full((max(self.entropy_stats()["subseqs_last"], 1), 4), -1, dtype=np.int32)
        h._ck(self.lib.yn_jpeg_entropy_states(h.h, self.j, int(i), out.ctypes.data, out.size), "yn_jpeg_entropy_states")
        return out[out[:, 0] >= 0].copy()

    def close(self):
        if getattr(self, "j", None):
            self.lib.yn_jpeg_destroy(self.j)
            self.j = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    info = staticmethod(info)

    def reason(self, i):
        return self.lib.yn_jpeg_reason(self.j, int(i)).decode()

    def timing(self, handle=None):
        """{'host_ms', 'h2d_ms', 'kernel_ms'} of the last batch (yn_jpeg_timing; synchronises): the host entropy stage of the whole batch,
        upload and kernels of its last chunk."""
        h = self._h(handle)
        ms = (ctypes.c_float * 3)()
        h._ck(self.lib.yn_jpeg_timing(h.h, self.j, ctypes.cast(ms, ctypes.c_void_p)), "yn_jpeg_timing")
        return {"host_ms": float(ms[0]), "h2d_ms": float(ms[1]), "kernel_ms": float(ms[2])}

    def decode_into(self, blobs, frames, handle=None):
        """yn_jpeg_decode_batch as it is: frames[i] a contiguous CUDA uint8 [h,w,3] tensor or None -> (statuses int32 [n], failed).
        Raises capi.YnError when the batch does not fit the staging slots."""
        h = self._h(handle)
        n = len(blobs)
        keep = [_buffer(b) for b in blobs]
        data = (ctypes.c_void_p * max(n, 1))(*[k[1] for k in keep])
        lens = np.array([k[2] for k in keep] + [0], dtype=np.int64)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[None if f is None else f.data_ptr() for f in frames])
        status = np.zeros(max(n, 1), dtype=np.int32)
        failed = ctypes.c_int()
        h._ck(self.lib.yn_jpeg_decode_batch(h.h, self.j, n, ctypes.cast(data, ctypes.c_void_p), lens.ctypes.data, ctypes.cast(ptrs, ctypes.c_void_p),
                                            status.ctypes.data, ctypes.byref(failed)), "yn_jpeg_decode_batch")
        return status[:n], int(failed.value)

    def batch(self, blobs, errors="raise", handle=None):
        """A list of JPEG files (bytes-like) -> a list of CUDA uint8 [h,w,3] BGR tensors.  A refused file raises ValueError naming its
        index and the reason; with errors="none" its entry is None and the others are decoded.  Asynchronous on the handle's stream with
        entropy="host"; with entropy="device" it waits, per chunk, for the entropy kernels' result words."""
        import torch
        assert errors in ("raise", "none")
        h = self._h(handle)
        h.follow_current_stream()
        metas = [info(b) for b in blobs]
        if errors == "raise":
            for i, m in enumerate(metas):
                if m["status"]:
                    raise ValueError("JPEG %d is %s: %s" % (i, STATUS_NAMES.get(m["status"], "refused"), m["reason"]))
        need = 0
        for c0 in range(0, len(blobs), self.max_batch):
            need = max(need, sum(2 * coefficient_count(m) for m in metas[c0:c0 + self.max_batch] if not m["status"]))
            if self.entropy == "device":                       # the scans are staged too: never more than the files themselves
                need = max(need, sum(-(-len(b) // 16) * 16 for b, m in zip(blobs[c0:c0 + self.max_batch], metas[c0:c0 + self.max_batch]) if not m["status"]))
        if need > self.staging_bytes:
            self._create(max(need, 2 * self.staging_bytes))
        frames = [None if m["status"] else torch.empty((m["h"], m["w"], 3), dtype=torch.uint8, device=h.device) for m in metas]
        status, failed = self.decode_into(blobs, frames, handle=h)
        if failed:
            bad = [i for i in range(len(blobs)) if status[i]]
            if errors == "raise":
                raise ValueError("JPEG %d is %s: %s" % (bad[0], STATUS_NAMES.get(int(status[bad[0]]), "refused"), self.reason(bad[0])))
            for i in bad:
                frames[i] = None
        return frames


_default = {}


def _decoder(device=None):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev not in _default:
        _default[dev] = JPEGDecoder(device=dev)
    return _default[dev]


def _read(src):
    if isinstance(src, (bytes, bytearray, memoryview, np.ndarray)):
        return src
    with open(src, "rb") as f:
        return f.read()


def imread(path_or_bytes, device=None):
    """cv2.imread(path) on the device: one uint8 [h,w,3] BGR CUDA tensor.  Raises ValueError for a file the decoder refuses."""
    return _decoder(device).batch([_read(path_or_bytes)])[0]


def imread_batch(paths, device=None, errors="raise"):
    """imread for a list of paths (or bytes objects), decoded together."""
    return _decoder(device).batch([_read(p) for p in paths], errors=errors)


# ---- the writer: cv2.imwrite(path_jpg, frame) on the device (yn_jpeg_enc_* / yn_jpeg_encode_*) ------------------------------
SAMPLINGS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
HEADER_BYTES = 623


def _sampling(sampling):
    if sampling in SAMPLINGS:
        return SAMPLINGS[sampling]
    if sampling in (0, 1, 2):
        return int(sampling)
    raise ValueError("sampling %r is not one of %s" % (sampling, ", ".join(sorted(SAMPLINGS))))


def quant_tables(quality):
    """jpeg_set_quality(quality, TRUE) (yn_jpeg_quant_tables; host only) -> uint16 [2, 64]: luma and chroma, natural order."""
    qt = np.zeros((2, 64), dtype=np.uint16)
    if capi.load_library().yn_jpeg_quant_tables(int(quality), qt.ctypes.data):
        raise ValueError("quality %r outside 1..100" % (quality,))
    return qt


def header(w, h, quality=95, sampling="4:2:0"):
    """The 623 bytes libjpeg writes before the entropy-coded data (yn_jpeg_header; host only)."""
    out = np.zeros(HEADER_BYTES, dtype=np.uint8)
    if capi.load_library().yn_jpeg_header(int(w), int(h), int(quality), _sampling(sampling), out.ctypes.data):
        raise ValueError("no header for %r x %r at quality %r" % (w, h, quality))
    return out.tobytes()


class JPEGEncoder(object):
    """A yn_jpeg_enc object: frames (CUDA uint8 [h,w,3] BGR tensors, as imread and Visualizer.batch produce) -> the bytes of the files
    cv2.imwrite / PIL write from them with libjpeg's defaults.  The whole encoder runs on the device; the finished files are what comes
    down.  The output buffer grows by itself (the object is recreated and the chunk runs again).
    Parity with the file cv2 itself writes is unpinned, because cv2 is not in the image: PIL runs the same libjpeg with the same defaults."""

    def __init__(self, max_batch=32, quality=95, sampling="4:2:0", handle=None, device=None, stream_bytes=None):
        self.lib = capi.load_library()
        self.max_batch, self.quality, self.sampling = int(max_batch), int(quality), sampling
        _sampling(sampling)
        self._handle, self._device = handle, device
        self.e = None
        self.stream_bytes = 0
        self._pinned = None
        self._n, self._geom, self._samp = 0, [], _sampling(sampling)      # the last encode(): nothing yet, fetch() gives []
        self._create(int(stream_bytes) if stream_bytes else max(self.max_batch * 640 * 480 * 3 // 4, 1 << 16))      # a quarter of VGA frames to begin with

    _h = JPEGDecoder._h

    def _create(self, stream_bytes, handle=None):
        h = self._h(handle)                                    # the object belongs to this handle's device
        keep = self._pinned                                    # the landing buffer outlives a regrow
        self.close()
        self._n, self._geom, self._pinned = 0, [], keep
        e = ctypes.c_void_p()
        h._ck(self.lib.yn_jpeg_enc_create(h.h, self.max_batch, int(stream_bytes), ctypes.byref(e)), "yn_jpeg_enc_create")
        self.e, self.stream_bytes = e, int(stream_bytes)

    def close(self):
        if getattr(self, "e", None):
            self.lib.yn_jpeg_enc_destroy(self.e)
            self.e = None
        self._pinned = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode(self, frames, quality=None, sampling=None, handle=None):
        """yn_jpeg_encode_batch as it is (at most max_batch frames, asynchronous).  Raises capi.YnError for a refused batch."""
        h = self._h(handle)
        n = len(frames)
        for i, f in enumerate(frames):
            if not (f.is_cuda and str(f.dtype) == "torch.uint8" and f.dim() == 3 and f.shape[2] == 3 and f.is_contiguous()):
                raise ValueError("frame %d is not a contiguous CUDA uint8 [h,w,3] tensor" % i)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[f.data_ptr() for f in frames])
        geom = np.array([[f.shape[1], f.shape[0]] for f in frames] + [[0, 0]], dtype=np.int32)
        h._ck(self.lib.yn_jpeg_encode_batch(h.h, self.e, n, ctypes.cast(ptrs, ctypes.c_void_p), geom.ctypes.data,
                                            self.quality if quality is None else int(quality), _sampling(self.sampling if sampling is None else sampling)),
              "yn_jpeg_encode_batch")
        self._n, self._geom = n, [(int(g[0]), int(g[1])) for g in geom[:n]]
        self._samp = _sampling(self.sampling if sampling is None else sampling)

    def fetch(self, handle=None):
        """yn_jpeg_encode_fetch -> the files of the last encode() as a list of bytes.  Raises capi.YnError when an image did not fit.
        The pinned landing buffer follows the files (a quarter more than the largest batch so far), not the encoder's capacity."""
        import torch
        h = self._h(handle)
        if self._pinned is None:
            self._pinned = torch.empty(min(self.stream_bytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
        offsets = np.zeros(self._n + 1, dtype=np.int64)
        rc = self.lib.yn_jpeg_encode_fetch(h.h, self.e, offsets.ctypes.data, self._pinned.data_ptr(), self._pinned.numel())
        if rc == 1 and "the caller's buffer" in self.lib.yn_last_error(h.h).decode():      # offsets are filled: make room, fetch again
            self._pinned = torch.empty(int(offsets[self._n]) + int(offsets[self._n]) // 4, dtype=torch.uint8, pin_memory=True)
            rc = self.lib.yn_jpeg_encode_fetch(h.h, self.e, offsets.ctypes.data, self._pinned.data_ptr(), self._pinned.numel())
        h._ck(rc, "yn_jpeg_encode_fetch")
        blob = self._pinned.numpy()
        return [blob[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(self._n)]

    def coefficients(self, i, handle=None):
        """The quantised coefficients of image i of the last encode() (yn_jpeg_enc_coefficients), as `coefficients` returns a file's:
        [int16 [bh, bw, 64] per component], natural order, MCU-padded grids."""
        h = self._h(handle)
        w, hh = self._geom[i]
        hs, vs = {0: (1, 1), 1: (2, 1), 2: (2, 2)}[self._samp]
        mw, mh = -(-w // (8 * hs)), -(-hh // (8 * vs))
        grids = [(mh * vs, mw * hs), (mh, mw), (mh, mw)]
        flat = np.zeros(64 * sum(a * b for a, b in grids), dtype=np.int16)
        h._ck(self.lib.yn_jpeg_enc_coefficients(h.h, self.e, int(i), flat.ctypes.data, flat.size), "yn_jpeg_enc_coefficients")
        out, off = [], 0
        for a, b in grids:
            out.append(flat[off:off + 64 * a * b].reshape(a, b, 64))
            off += 64 * a * b
        return out

    def guard_intact(self, handle=None):
        """True while the 64 bytes behind the output buffer are untouched (yn_jpeg_enc_guard)."""
        h = self._h(handle)
        g = np.zeros(64, dtype=np.uint8)
        h._ck(self.lib.yn_jpeg_enc_guard(h.h, self.e, g.ctypes.data), "yn_jpeg_enc_guard")
        return bool((g == 0xA5).all())

    def timing(self, handle=None):
        """Milliseconds of the last encode() per stage (yn_jpeg_enc_timing; synchronises)."""
        h = self._h(handle)
        ms = (ctypes.c_float * 10)()
        h._ck(self.lib.yn_jpeg_enc_timing(h.h, self.e, ctypes.cast(ms, ctypes.c_void_p)), "yn_jpeg_enc_timing")
        return dict(zip(("upload_clear", "fdct", "bits", "scan_tiles", "scan_sums_layout", "emit", "ff_count", "ff_scan_tiles", "ff_scan_sums_layout", "files"),
                        [float(v) for v in ms]))

    def batch(self, frames, quality=None, sampling=None, handle=None):
        """A list of frames -> a list of bytes objects, each a complete JPEG file.  More than max_batch frames are encoded in chunks."""
        import re
        h = self._h(handle)
        h.follow_current_stream()
        q = self.quality if quality is None else int(quality)
        s = _sampling(self.sampling if sampling is None else sampling)
        out = []
        for c0 in range(0, len(frames), self.max_batch):
            chunk = list(frames[c0:c0 + self.max_batch])
            while True:
                self.encode(chunk, q, s, handle=h)
                try:
                    out += self.fetch(handle=h)
                    break
                except capi.YnError as err:
                    m = re.search(r"needs (\d+) output bytes and (\d+) stream bytes", str(err))
                    if m is None:
                        raise
                    self._create(max(2 * self.stream_bytes, int(m.group(1)) + int(m.group(1)) // 64 + 1024, int(m.group(2))), handle=h)
        return out


_default_enc = {}


def _encoder(device=None):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev not in _default_enc:
        _default_enc[dev] = JPEGEncoder(device=dev)
    return _default_enc[dev]


def imencode(frame, quality=95, sampling="4:2:0"):
    """cv2.imencode(".jpg", frame) on the device: the bytes of the file."""
    return _encoder(frame.device).batch([frame], quality=quality, sampling=sampling)[0]


def imwrite(path, frame, quality=95, sampling="4:2:0"):
    """cv2.imwrite(path_jpg, frame) for a CUDA uint8 [h,w,3] BGR frame."""
    with open(path, "wb") as f:
        f.write(imencode(frame, quality=quality, sampling=sampling))


def imwrite_batch(paths, frames, quality=95, sampling="4:2:0"):
    """imwrite for a list of paths and frames, encoded together."""
    assert len(paths) == len(frames)
    files = _encoder(frames[0].device).batch(list(frames), quality=quality, sampling=sampling) if frames else []
    for p, b in zip(paths, files):
        with open(p, "wb") as f:
            f.write(b)
