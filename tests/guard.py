"""Guard bands around every device buffer of a C-ABI call (a plain helper module: tests/test_ws_sections.py, tests/test_gpu_guard_bands.py).

torch's caching allocator rounds every request up and hands out pieces of larger blocks, so a store a few rows past the end of `grad` or
of the workspace lands in slack nobody reads.  Here ONE uint8 tensor filled with 0xFF (every float in it reads as NaN, every int32 as -1)
is the `Arena`; every buffer of a call is carved from it with 64 KiB of untouched bytes on each side -- two rows of the largest supported
V = 8192 in fp32, wider than any single row a kernel stores -- and the workspace is exactly as large as the library says it needs, with
the map of its sections (crf_debug_ws_sections) telling which bytes inside it belong to no section: the padding up to the next multiple
of 256 and, with the switch ws_gap, n x 256 more behind every section.  `Arena.check` asserts that all of these are still 0xFF.  The NaN
bands around the activations double as a read check: a kernel that uses an element beyond the last row produces NaN or misses the oracle.

The drivers call the C ABI through `_C._lib` -- not the product path of `_C.loss_fwd_bwd`, which allocates through torch."""
import ctypes

import numpy as np
import torch

GUARD = 64 * 1024
DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
SENT_POS, SENT_SCORE = -77, 12345.0


class GuardError(AssertionError):
    """A guard band or a gap of the workspace is no longer 0xFF: `name` of the buffer or section, `side` ("before" / "after"), `first` /
    `last` corrupted byte as offsets from the START of that buffer or section (negative in front of it, >= its size behind it)."""

    def __init__(self, name, side, first, last, nbytes):
        self.name, self.side, self.first, self.last, self.nbytes = name, side, first, last, nbytes
        super().__init__(f"{name} ({nbytes} bytes): bytes {side} it were written, offsets [{first}, {last}] from its start")


def _roundup(x, a):
    return (x + a - 1) // a * a


class Arena:
    def __init__(self, device, nbytes):
        self.buf = torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device=device)
        self.top = 0          # first byte no carve or band has claimed
        self.carves = {}      # name -> (start, nbytes, start of the band in front)

    @staticmethod
    def room(sizes, align=256):
        """Bytes an arena needs for carves of these sizes (with any misalign < align)."""
        return sum(2 * GUARD + 2 * align + int(n) for n in sizes) + 512

    def carve(self, name, nbytes, align=256, misalign=0):
        """A uint8 view of `nbytes` whose address is `misalign` past a multiple of `align`, at least 64 KiB behind everything carved so
        far and followed by 64 KiB of its own."""
        assert name not in self.carves and 0 <= misalign < align
        base = self.buf.data_ptr()
        start = _roundup(base + self.top + GUARD, align) - base + misalign
        end = start + int(nbytes)
        assert end + GUARD <= self.buf.numel(), "arena too small"
        self.carves[name] = (start, int(nbytes), self.top)
        self.top = end + GUARD
        return self.buf[start:end]

    def view(self, name):
        start, n, _ = self.carves[name]
        return self.buf[start:start + n]

    def ptr(self, name):
        return ctypes.c_void_p(self.buf.data_ptr() + self.carves[name][0])

    def put(self, name, t):
        """Copy a tensor's bytes into its carve (a torch op on the current stream)."""
        src = t.contiguous().reshape(-1).view(torch.uint8)
        assert src.numel() == self.carves[name][1], (name, src.numel(), self.carves[name][1])
        if src.numel():
            self.view(name).copy_(src.to(self.buf.device), non_blocking=False)

    def get(self, name, dtype, shape=None):
        """The carve's bytes as a fresh CPU tensor of `dtype`."""
        t = self.view(name).clone().view(dtype)
        return (t if shape is None else t.reshape(shape)).cpu()

    def bands(self, sections=None, ws="ws"):
        """[(name, nbytes of it, side, band start, band end, start of the buffer or section)] in arena offsets: the two bands of every
        carve, and for the carve `ws` the bytes between the end of every section and the start of the next one (the end of the carve
        after the last)."""
        out = []
        for name, (start, n, lo) in self.carves.items():
            out.append((name, n, "before", lo, start, start))
            out.append((name, n, "after", start + n, start + n + GUARD, start))
        if sections is not None:
            w0, wn, _ = self.carves[ws]
            secs = list(sections)
            for k, (sname, off, nb) in enumerate(secs):
                nxt = secs[k + 1][1] if k + 1 < len(secs) else wn
                assert 0 <= off and off + nb <= nxt <= wn, ("sections overlap or leave the workspace", sname, off, nb, nxt, wn)
                out.append((f"{ws}.{sname}", nb, "after", w0 + off + nb, w0 + nxt, w0 + off))
            assert secs[0][1] == 0, "the first section starts the workspace"
        return [b for b in out if b[4] > b[3]]

    def check(self, sections=None, ws="ws"):
        """Every guard byte (and, with the workspace's section map, every byte of `ws` outside its sections) is still 0xFF: one
        device-side comparison per band, one word per band copied to the host."""
        bands = self.bands(sections, ws)
        flags = torch.stack([(self.buf[lo:hi] != 0xFF).any() for _, _, _, lo, hi, _ in bands]).cpu().numpy()
        for bad, (name, n, side, lo, hi, origin) in zip(flags, bands):
            if bad:
                idx = torch.nonzero(self.buf[lo:hi] != 0xFF).reshape(-1)
                raise GuardError(name, side, lo + int(idx[0]) - origin, lo + int(idx[-1]) - origin, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# drivers: one call of the C ABI on carved buffers
# ---------------------------------------------------------------------------------------------------------------------------------
def _i32(a):
    return torch.tensor(np.asarray(a).reshape(-1), dtype=torch.int32)


def _meta(arena, labels, lx, ly):
    ly_t = _i32(ly)
    off = torch.cumsum(ly_t, 0, dtype=torch.int32) - ly_t
    for name, t in (("labels", _i32(labels)), ("lab_off", off), ("lx", _i32(lx)), ("ly", ly_t)):
        arena.carve(name, 4 * t.numel())
        arena.put(name, t)
    return int(ly_t.max()) if ly_t.numel() else 0


def run_loss(core, graph, x, labels, lx, ly, c_den, c_ctc, fused=False, time_major=False, blank=0, null_outputs=False, misalign=0):
    """crf_loss_fwd_bwd / crf_loss_fwd_bwd_logits (graph: a handle) or crf_ctc_fwd_bwd / crf_ctc_fwd_bwd_logits (graph None) on carved
    buffers, under whatever switches are set.  x: CPU tensor [B,T,V] ([T,B,V] time-major), fp32 log-probs or -- fused -- raw output in
    fp32 / bf16 / fp16; misalign: bytes the activations start past a multiple of 256.  null_outputs: the three cost vectors and
    `invalid` are NULL.  Checks the bands, then returns dict(loss, grad [x's shape], costs_den, costs_beta, costs_ctc, invalid) as numpy
    (None for a NULL output), plus kernel = last_den_kernel(), streams, fallbacks = last_fallback_counts() and the workspace's sections."""
    dev = torch.device("cuda", 0)
    B, T, V = (x.shape[1], x.shape[0], x.shape[2]) if time_major else x.shape
    assert fused or x.dtype == torch.float32
    vp = ctypes.c_void_p
    gh = vp(graph or 0)
    max_l = int(np.max(ly)) if len(ly) else 0
    nws = core._lib.crf_workspace_bytes(gh, B, T, V, max_l)
    assert nws > 0
    sections = core.debug_ws_sections(graph, B, T, V, max_l)
    esz = x.element_size()
    outs = [] if null_outputs else [(n, 4 * B) for n in (("costs_den", "costs_beta") if graph else ()) + ("costs_ctc", "invalid")]
    arena = Arena(dev, Arena.room([x.numel() * esz, 4 * len(np.asarray(labels).reshape(-1)), 4 * B, 4 * B, 4 * B, 4 * x.numel(), 4, nws] +
                                  [n for _, n in outs]))
    arena.carve("act", x.numel() * esz, misalign=misalign)
    arena.put("act", x)
    assert _meta(arena, labels, lx, ly) == max_l
    arena.carve("grad", 4 * x.numel())
    arena.carve("loss", 4)
    for name, n in outs:
        arena.carve(name, n)
    arena.carve("ws", nws)
    P = lambda name: arena.ptr(name) if name in arena.carves else vp(0)
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    tail = (P("labels"), P("lab_off"), P("lx"), P("ly"), B, T, V, max_l)
    with torch.cuda.device(dev):
        if graph is None:
            assert c_den == 0.0
            head = (P("act"), DTYPES[x.dtype]) if fused else (P("act"),)
            fn = core._lib.crf_ctc_fwd_bwd_logits if fused else core._lib.crf_ctc_fwd_bwd
            rc = fn(*head, 1 if time_major else 0, blank, *tail, c_ctc, P("grad"), P("loss"), P("costs_ctc"), P("invalid"), P("ws"), nws, stream)
        else:
            assert not time_major and blank == 0
            head = (gh, P("act"), DTYPES[x.dtype]) if fused else (gh, P("act"))
            fn = core._lib.crf_loss_fwd_bwd_logits if fused else core._lib.crf_loss_fwd_bwd
            rc = fn(*head, *tail, c_den, c_ctc, P("grad"), P("loss"), P("costs_den"), P("costs_beta"), P("costs_ctc"), P("invalid"), P("ws"),
                    nws, stream)
    assert rc == 0, core._lib.crf_last_error().decode()
    kernel, streams = core.last_den_kernel(), core.last_call_streams()
    falls = core.last_fallback_counts(torch.cuda.current_stream(dev).cuda_stream)   # (synchronises the stream; the words live in this workspace)
    torch.cuda.synchronize()
    arena.check(sections)
    assert bool((arena.view("ws")[:sections[0][2]] != 0xFF).any()), "the call did not use the carved workspace"
    assert torch.equal(arena.get("act", torch.uint8), x.contiguous().reshape(-1).view(torch.uint8)), "the call wrote to its input"
    f = lambda name: arena.get(name, torch.float32).numpy() if name in arena.carves else None
    return dict(loss=float(arena.get("loss", torch.float32)[0]), grad=arena.get("grad", torch.float32, tuple(x.shape)).numpy(),
                costs_den=f("costs_den"), costs_beta=f("costs_beta"), costs_ctc=f("costs_ctc"),
                invalid=arena.get("invalid", torch.int32).numpy() if "invalid" in arena.carves else None, kernel=kernel, streams=streams,
                fallbacks=falls, sections=sections)


def run_align(core, x, labels, lx, ly, blank, fused=False, time_major=False, misalign=0):
    """crf_ctc_align (x: fp32 log-probs) / crf_ctc_align_logits (fused: raw output in fp32 / bf16 / fp16) on carved buffers; `pos` and
    `score` are prefilled with sentinels.  Checks the bands and that no sentinel is left -> (pos [B,T], score [B], invalid [B]) as numpy."""
    dev = torch.device("cuda", 0)
    B, T, V = (x.shape[1], x.shape[0], x.shape[2]) if time_major else x.shape
    assert fused or x.dtype == torch.float32
    vp = ctypes.c_void_p
    max_l = int(np.max(ly)) if len(ly) else 0
    nws = (core._lib.crf_ctc_align_logits_workspace_bytes if fused else core._lib.crf_ctc_align_workspace_bytes)(B, T, V, max_l)
    assert nws > 0
    sections = core.debug_align_ws_sections(fused, B, T, V, max_l)
    esz = x.element_size()
    arena = Arena(dev, Arena.room([x.numel() * esz, 4 * len(np.asarray(labels).reshape(-1)), 4 * B, 4 * B, 4 * B, 4 * B * T, 4 * B, 4 * B, nws]))
    arena.carve("act", x.numel() * esz, misalign=misalign)
    arena.put("act", x)
    assert _meta(arena, labels, lx, ly) == max_l
    arena.carve("pos", 4 * B * T)
    arena.put("pos", torch.full((B, T), SENT_POS, dtype=torch.int32))
    arena.carve("score", 4 * B)
    arena.put("score", torch.full((B,), SENT_SCORE, dtype=torch.float32))
    arena.carve("invalid", 4 * B)
    arena.carve("ws", nws)
    P = arena.ptr
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    head = (P("act"), DTYPES[x.dtype]) if fused else (P("act"),)
    fn = core._lib.crf_ctc_align_logits if fused else core._lib.crf_ctc_align
    with torch.cuda.device(dev):
        rc = fn(*head, 1 if time_major else 0, blank, P("labels"), P("lab_off"), P("lx"), P("ly"), B, T, V, max_l, P("pos"), P("score"),
                P("invalid"), P("ws"), nws, stream)
    assert rc == 0, core._lib.crf_last_error().decode()
    torch.cuda.synchronize()
    arena.check(sections)
    assert torch.equal(arena.get("act", torch.uint8), x.contiguous().reshape(-1).view(torch.uint8)), "the call wrote to its input"
    pos, sc = arena.get("pos", torch.int32, (B, T)).numpy(), arena.get("score", torch.float32).numpy()
    inv = arena.get("invalid", torch.int32).numpy()
    assert not np.any(pos == SENT_POS) and not np.any(sc == SENT_SCORE) and np.all((inv == 0) | (inv == 1))
    return pos, sc, inv
