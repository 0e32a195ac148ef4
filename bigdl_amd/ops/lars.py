"""Fused LARS on the GPU engine: every layer's norms and every layer's update in three launches (csrc/lars.hip).

A ``LarsPlan`` is built once from the update pieces that belong to ``LarsSGD`` methods. It holds the tables the
kernels read (pieces, chunks, the chunk range of every layer), the per-chunk partial workspace, the per-layer sums
``acc`` (2 floats per layer: sum w^2, sum g^2; what the ranks all-reduce), one flat fp32 momentum buffer that every
method's ``state["v"]`` is a view of, and the per-step rates (``-currentRate * trust`` of every piece), which reach
the device through two alternating pinned host buffers and a non-blocking copy: nothing in a step waits on the host.

Switch: ``BIGDL_LARS_FUSED`` / Engine property ``bigdl.lars.fused`` / ``set_fused``; unset means ``DEFAULT_FUSED``
for GPU tensors. ``last_route()`` says whether the last LARS update ran "fused" or through the per-layer "loop".
"""
import os
import weakref

import torch

from . import native

CHUNK = 4096            # BIGDL_LARS_CHUNK      (csrc/kernels.h): elements of one workgroup's chunk
BLOCK_CAP = 2048        # BIGDL_LARS_BLOCK_CAP: blocks of the norm and update grids
DEFAULT_FUSED = True    # the GPU engine's default (README "Fused LARS"; profiles/lars_fused_ab.txt)

_FUSED = [None]
_ROUTE = [None]


def set_fused(v):
    """True / False, "1" / "0", or None for the engine's default."""
    _FUSED[0] = None if v is None or v == "" else str(v).lower() in ("1", "true", "yes")


def fused(is_cuda=True):
    """Whether a caller with GPU tensors (``is_cuda``) takes the fused route."""
    v = _FUSED[0]
    if v is None:
        env = os.environ.get("BIGDL_LARS_FUSED", "")
        v = DEFAULT_FUSED if env == "" else env.lower() in ("1", "true", "yes")
    return bool(v) and bool(is_cuda)


def last_route():
    """"fused" or "loop": the route of the last LARS update (None before the first)."""
    return _ROUTE[0]


def _set_route(route):
    _ROUTE[0] = route


def phase_of(t):
    """Elements past a 16-byte boundary at which ``t`` starts (0..3 for fp32 / bf16 alike): the kernels split a chunk
    into head / 16-byte body / tail once for all buffers, so all of them must agree on it."""
    return (t.data_ptr() // t.element_size()) % 4


def build_tables(pieces, nlayers, chunk=CHUNK):
    """Host tables for ``pieces`` = [(lo, hi, layer)], layer ids in [0, nlayers).

    Chunks are numbered layer by layer (within a layer: pieces by ascending ``lo``, then ascending offset), so the
    chunks of a layer are one contiguous range ``layer_chunks[layer] = [first, end)`` and the finish kernel's order
    of summation is a function of the tables alone. A piece's momentum lives at ``lo + dv`` of the momentum buffer;
    ``dv`` is a multiple of 4, so w, g and v share the 16-byte phase of every element.
    """
    for lo, hi, layer in pieces:
        if not (0 <= lo < hi) or not (0 <= layer < nlayers):
            raise ValueError(f"LarsPlan: bad piece ({lo}, {hi}, layer {layer} of {nlayers})")
    piece_tab, cur = [], 0
    for lo, hi, layer in pieces:
        voff = cur + (lo - cur) % 4
        piece_tab.append((lo, hi, voff - lo, layer))
        cur = voff + (hi - lo)
    chunk_piece, chunk_start, layer_chunks = [], [], []
    order = sorted(range(len(pieces)), key=lambda i: (pieces[i][2], pieces[i][0]))
    k = 0
    for layer in range(nlayers):
        first = len(chunk_piece)
        while k < len(order) and pieces[order[k]][2] == layer:
            lo, hi, _ = pieces[order[k]]
            for s in range(lo, hi, chunk):
                chunk_piece.append(order[k])
                chunk_start.append(s)
            k += 1
        layer_chunks.append((first, len(chunk_piece)))
    return {"piece_tab": piece_tab, "chunk_piece": chunk_piece, "chunk_start": chunk_start,
            "layer_chunks": layer_chunks, "max_hi": max((p[1] for p in pieces), default=0), "v_need": cur}


def device_tables(tab, device):
    """The tables of ``build_tables`` as the device tensors the bindings take."""
    def t(v, dt, shape):          # through pinned memory: building a plan does not wait for the stream either
        h = torch.tensor(v, dtype=dt).reshape(shape)
        return h.pin_memory().to(device, non_blocking=True) if torch.device(device).type == "cuda" else h

    return {"piece_tab": t(tab["piece_tab"], torch.int64, (-1, 4)),
            "chunk_piece": t(tab["chunk_piece"], torch.int32, (-1,)),
            "chunk_start": t(tab["chunk_start"], torch.int64, (-1,)),
            "layer_chunks": t(tab["layer_chunks"], torch.int32, (-1, 2))}


class LarsPlan:
    """``pieces``: [(lo, hi, layer, method)] (method: the piece's own LarsSGD). ``phase``: the 16-byte phase of the
    weight buffer the plan will be run on (``phase_of``; 0 for a whole allocation)."""

    def __init__(self, pieces, nlayers, device, phase=0):
        C = native.get()
        assert (C.LARS_CHUNK, C.LARS_BLOCK_CAP) == (CHUNK, BLOCK_CAP)
        self.device = torch.device(device)
        self.methods = [p[3] for p in pieces]
        self.spans = [(int(p[0]), int(p[1]), int(p[2])) for p in pieces]
        self.nlayers = int(nlayers)
        self.tab = build_tables(self.spans, self.nlayers)
        self.dev = device_tables(self.tab, self.device)
        self.max_hi, self.v_need = self.tab["max_hi"], self.tab["v_need"]
        self.nchunks, npieces = len(self.tab["chunk_piece"]), len(pieces)
        self.phase = int(phase)
        self.ws = torch.empty(max(2 * self.nchunks, 1), dtype=torch.float32, device=self.device)
        self.acc = torch.zeros(max(2 * self.nlayers, 1), dtype=torch.float32, device=self.device)
        self.acc_fresh = False          # acc holds this step's sums (set by norms, cleared by update)
        self.vbuf = torch.zeros(self.v_need + 4, dtype=torch.float32, device=self.device)[phase:phase + self.v_need]
        self.views = [self.vbuf[lo + dv:hi + dv] for lo, hi, dv, _ in self.tab["piece_tab"]]
        self.rates = torch.zeros(max(npieces, 1), dtype=torch.float32, device=self.device)
        self._pin = [torch.zeros(max(npieces, 1), dtype=torch.float32).pin_memory() for _ in range(2)]
        self._pin_np = [b.numpy() for b in self._pin]
        self._pin_ev = [None, None]
        self._flip = 0
        self._hp = None
        self.piece_hp = torch.zeros(max(npieces, 1) * 2, dtype=torch.float32, device=self.device)[:2 * npieces]

    # ------------------------------------------------------------------ per-step host work
    def usable(self, w, g, w16=None):
        """The buffers cover the pieces and share the plan's 16-byte phase."""
        ok = w.numel() >= self.max_hi and g.numel() >= self.max_hi and phase_of(w) == self.phase == phase_of(g)
        return ok and (w16 is None or (w16.numel() >= self.max_hi and phase_of(w16) == self.phase))

    def bind_state(self):
        """Every method's ``state["v"]`` is the plan's view of its piece: a missing one (first step, clearHistory) is
        zero-filled, a foreign one (a loaded checkpoint, a value set by hand) is copied in; both are then re-viewed."""
        for m, view in zip(self.methods, self.views):
            sv = m.state.get("v")
            if torch.is_tensor(sv) and sv.data_ptr() == view.data_ptr() and sv.numel() == view.numel():
                continue
            if sv is None:
                view.zero_()
            else:
                if sv.numel() != view.numel():
                    raise ValueError(f"LarsSGD state v has {sv.numel()} elements, its piece has {view.numel()}")
                view.copy_(sv.reshape(-1), non_blocking=True)
            m.state["v"] = view

    def _put_hp(self):
        hp = [float(x) for m in self.methods for x in (m.weightDecay, m.momentum)]
        if hp != self._hp:              # a schedule may rewrite them (EpochSchedule regimes): rare
            self._hp = hp
            if hp:
                self.piece_hp.copy_(torch.tensor(hp, dtype=torch.float32).pin_memory(), non_blocking=True)

    def put_rates(self, rates):
        """Per-piece ``-currentRate * trust`` to the device array. The two pinned buffers alternate, and a buffer is
        refilled only after the copy that last read it has run (an event query; a host far ahead polls)."""
        i = self._flip
        self._flip ^= 1
        ev = self._pin_ev[i]
        if ev is not None and not ev.query():
            from ..optim.train_step import wait_event

            wait_event(ev)
        self._pin_np[i][:len(rates)] = rates
        self.rates.copy_(self._pin[i], non_blocking=True)
        if ev is None:
            ev = self._pin_ev[i] = torch.cuda.Event()
        ev.record()

    def advance(self):
        """Advance every method's schedule on the host, as ``LarsSGD.optimize`` does, and publish the rates."""
        rates = []
        for m in self.methods:
            m.learningRateSchedule.updateHyperParameter(m)
            rates.append(-m.learningRateSchedule.currentRate * m.trust)
        self.put_rates(rates)

    # ------------------------------------------------------------------ launches
    def norms(self, w, g):
        """Two launches: acc[2 l], acc[2 l + 1] = this rank's sum w^2, sum g^2 of layer l."""
        d = self.dev
        native.get().lars_norms(w, g, d["chunk_piece"], d["chunk_start"], d["piece_tab"], d["layer_chunks"], self.ws,
                                self.acc, self.max_hi)
        self.acc_fresh = True

    def update(self, w, g, w16, WD, acc=None):
        """One launch over every piece; ``acc`` defaults to the plan's own (all-reduced) sums."""
        d = self.dev
        self.bind_state()
        self._put_hp()
        native.get().lars_update(w, g, self.vbuf, w16, d["chunk_piece"], d["chunk_start"], d["piece_tab"],
                                 self.piece_hp, self.rates, self.acc if acc is None else acc, float(WD), self.max_hi,
                                 self.v_need, self.nlayers)
        self.acc_fresh = False
        _set_route("fused")


_ONE = weakref.WeakKeyDictionary()      # LarsSGD -> its cached one-piece plan (stand-alone optimize)


def one_piece_plan(method, x):
    """The cached plan of a stand-alone ``LarsSGD.optimize(feval, x)``: one piece [0, n), one layer."""
    key = (x.numel(), x.device, phase_of(x))
    got = _ONE.get(method)
    if got is None or got[0] != key:
        got = (key, LarsPlan([(0, x.numel(), 0, method)], 1, x.device, phase=key[2]))
        _ONE[method] = got
    return got[1]


__all__ = ["CHUNK", "BLOCK_CAP", "DEFAULT_FUSED", "set_fused", "fused", "last_route", "phase_of", "build_tables",
           "device_tables", "LarsPlan", "one_piece_plan"]
