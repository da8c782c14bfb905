"""Sinsemilla over Pallas in bulk (halo2_amd/csrc/sinsemilla.hip): the hash of Orchard's note-commitment tree (MerkleCRH) and the
witness of the Sinsemilla chip.  Zcash protocol specification 5.4.1.9: K = 10, C = 253,
    S(j) = hash_to_curve("z.cash:SinsemillaS")(j as 4 bytes LE),   Q(D) = hash_to_curve("z.cash:SinsemillaQ")(D),
    hash_to_point(m_1 .. m_n) = fold Acc <- (Acc + S(m_i)) + Acc from Q, with INCOMPLETE addition: a chain that meets equal or
    opposite operands has no value (the reference's `None`), reported here per message.

Field elements and points are arrays of uint64 Montgomery limbs ((..., 4) and (..., 8)): a CUDA int64 tensor is used in place and a
CUDA tensor comes back; a numpy array is uploaded and a numpy array comes back.  The 1024-point table S is built once per process and
device by h2_hash_to_curve_device and stays in HBM (64 KiB).

`CommitDomain` is the `sinsemilla` crate's: SinsemillaCommit and SinsemillaShortCommit (specification 5.4.8.4), hash and blinding
product in one launch (halo2_amd/csrc/sinsemilla_commit.hip).  `HashDomain.hash_to_point(.., Q=)` and `trace_from` start every message
from a point of its own: the reference's hash_to_point_with_private_init."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import fields
from ._lib import FORM_MONTGOMERY, check, lib
from .arithmetic import _is_torch, _p, _stream_ptr

__all__ = ["K", "C_MAX", "HashDomain", "generator_table", "generator_table_ints", "q_point", "merkle_crh", "merkle_root", "trace",
           "trace_from", "CommitDomain", "Bottom", "MERKLE_CRH_DOMAIN", "merkle_paths", "merkle_path_trace", "MerklePathTrace",
           "MERKLE_PIECE_WORDS", "MAX_MERKLE_DEPTH"]

K = 10
C_MAX = 253                                     # the specification's C: words per message
S_PERSONALIZATION = "z.cash:SinsemillaS"
Q_PERSONALIZATION = "z.cash:SinsemillaQ"
MERKLE_CRH_DOMAIN = "z.cash:Orchard-MerkleCRH"
PALLAS, FP = 0, 0

_tables: dict = {}
_table_ints: dict = {}


class Bottom(ValueError):
    """A Sinsemilla hash met an exceptional addition: the specification's bottom."""


def generator_table():
    """S(0) .. S(1023) as a (1024, 8) int64 CUDA tensor of Montgomery affine limbs on the current device; built on first use, on the
    stream current then.  The build is asynchronous, so the table is cached with an event recorded behind it: a caller on another
    stream is made to wait for that event, until the event is seen complete once and dropped (steady-state calls pay one dict look-up)."""
    import torch
    dev = fields.current_device()
    if dev.index not in _tables:
        msgs = torch.from_numpy(np.arange(1 << K, dtype="<u4").view(np.uint8).reshape(1 << K, 4).copy()).to(dev)
        out = torch.empty((1 << K, 8), dtype=torch.int64, device=dev)
        check(lib().h2_hash_to_curve_device(PALLAS, S_PERSONALIZATION.encode(), msgs.data_ptr(), 4, 1 << K, FORM_MONTGOMERY,
                                            out.data_ptr(), _stream_ptr()), "h2_hash_to_curve_device")
        built = torch.cuda.Event()
        built.record(torch.cuda.current_stream(dev))
        _tables[dev.index] = (out, built)
    out, built = _tables[dev.index]
    if built is not None:
        if built.query():
            _tables[dev.index] = (out, None)
        else:
            torch.cuda.current_stream(dev).wait_event(built)
    return out


def _points_to_ints(limbs) -> list:
    v = fields.from_limbs(np.asarray(limbs).reshape(-1, 4), FP)
    return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]


def generator_table_ints(table=None) -> list:
    """The table as 1024 (x, y) pairs of Python integers: `table` if given (a list of pairs, or (1024, 8) Montgomery limbs), the device's
    otherwise.  This is what the chip's synthesis reads."""
    if table is None:
        index = fields.current_device().index
        if index not in _table_ints:
            _table_ints[index] = _points_to_ints(generator_table().cpu().numpy().view(np.uint64))
        return _table_ints[index]
    if isinstance(table, np.ndarray):
        return _points_to_ints(table)
    table = [(int(x), int(y)) for x, y in table]
    if len(table) != 1 << K:
        raise ValueError("sinsemilla: the table has 2^10 points")
    return table


def _device_table(table):
    """-> (1024, 8) int64 CUDA tensor from an injected table, or the process's own"""
    import torch
    if table is None:
        return generator_table()
    if _is_torch(table):
        return table.contiguous()
    if not isinstance(table, np.ndarray):
        table = fields.to_limbs([c for pt in table for c in pt], FP).reshape(-1, 8)
    if table.shape != (1 << K, 8):
        raise ValueError("sinsemilla: the table has 2^10 points")
    return torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint64).view(np.int64)).to(fields.current_device())


def q_point(domain) -> tuple:
    """Q(D) = hash_to_curve("z.cash:SinsemillaQ")(D) as (x, y) integers."""
    from .commitment import hash_to_curve
    d = domain.encode() if isinstance(domain, str) else bytes(domain)
    return _points_to_ints(hash_to_curve(PALLAS, Q_PERSONALIZATION, [d]))[0]


def _q_limbs(q) -> np.ndarray:
    return np.ascontiguousarray(fields.to_limbs([q[0], q[1]], FP).reshape(8))


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _raise_bottom(status, what):
    bad = status.nonzero().flatten()
    if bad.numel():
        raise Bottom(f"{what}: message {int(bad[0])} meets an exceptional addition ({bad.numel()} of {status.numel()} do)")


def _device_words(words, what):
    """-> ((n, len) int16 CUDA tensor, whether `words` came from the host)"""
    import torch
    host = not _is_torch(words)
    if host:
        w = np.asarray(words)
        if w.ndim != 2 or (w.size and (w.min() < 0 or w.max() >= 1 << K)):
            raise ValueError(f"{what}: an (n, len) array of 10-bit words")
        w = torch.from_numpy(np.ascontiguousarray(w, dtype=np.uint16).view(np.int16)).to(fields.current_device())
    else:
        w = words.contiguous()
        if w.dtype != torch.int16 or w.ndim != 2 or not w.is_cuda:
            raise ValueError(f"{what}: an (n, len) CUDA int16 tensor of 10-bit words")
    if w.shape[1] > C_MAX:
        raise ValueError(f"{what}: a message has at most 253 words")
    return w, host


def _device_limbs(a, n, width, host, what):
    """-> (n, width) int64 CUDA tensor from an array of the kind of the call's first argument"""
    import torch
    if host == _is_torch(a):
        raise ValueError(f"{what}: every argument of one kind, numpy arrays or CUDA tensors")
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(fields.current_device()) if host else a.contiguous()
    if t.shape != (n, width) or t.dtype != torch.int64 or not t.is_cuda:
        raise ValueError(f"{what}: an ({n}, {width}) array of uint64 limbs")
    return t


def _device_points(q, n, host, what):
    return _device_limbs(q, n, 8, host, what + " Q")


class HashDomain:
    """`HashDomain::new(name)` (halo2_gadgets/src/sinsemilla.rs), or a domain with a caller's Q: `HashDomain((x, y))`.
    `table=` replaces the generator table (host tests inject one computed on the CPU)."""

    def __init__(self, name_or_q, table=None):
        self.Q = q_point(name_or_q) if isinstance(name_or_q, (str, bytes)) else (int(name_or_q[0]), int(name_or_q[1]))
        self.table = table

    def hash_to_point(self, words, with_status: bool = False, Q=None):
        """n messages of `len` words (< 1024): an (n, len) integer array or CUDA int16 tensor -> (n, 8) affine points.  A message without
        a value raises `Bottom`; with_status: returns (points, status) instead -- status[i] = 1 and a zero point for such a message.
        Q: (n, 8) Montgomery affine points, of the kind of `words`: message i starts from Q[i] instead of the domain's Q."""
        import torch
        w, host = _device_words(words, "sinsemilla.hash_to_point")
        n, length = w.shape
        tab = _device_table(self.table)
        out = torch.empty((n, 8), dtype=torch.int64, device=w.device)
        status = torch.empty((n,), dtype=torch.uint8, device=w.device)
        if Q is None:
            check(lib().h2_sinsemilla_hash_device(_ptr(w), n, length, _p(_q_limbs(self.Q)), tab.data_ptr(), _ptr(out), _ptr(status),
                                                  _stream_ptr()), "h2_sinsemilla_hash_device")
        else:
            q = _device_points(Q, n, host, "sinsemilla.hash_to_point")
            check(lib().h2_sinsemilla_hash_from_device(_ptr(w), n, length, _ptr(q), tab.data_ptr(), _ptr(out), _ptr(status), _stream_ptr()),
                  "h2_sinsemilla_hash_from_device")
        if with_status:
            return (out.cpu().numpy().view(np.uint64), status.cpu().numpy()) if host else (out, status)
        _raise_bottom(status, "sinsemilla.hash_to_point")
        return out.cpu().numpy().view(np.uint64) if host else out

    def hash(self, words):                                                    # noqa: A003 -- the reference's name
        """The x coordinates of hash_to_point: (n, len) -> (n, 4)."""
        pts = self.hash_to_point(words)
        return np.ascontiguousarray(pts[:, :4]) if isinstance(pts, np.ndarray) else pts[:, :4].contiguous()


def _merkle_domain(domain):
    if domain is None:
        return HashDomain(MERKLE_CRH_DOMAIN)
    return domain if isinstance(domain, HashDomain) else HashDomain(domain)


def merkle_crh(layer: int, left, right, domain=None):
    """MerkleCRH (specification 5.4.1.3) of n pairs: the hash of  layer (10 bits) || left (255 bits) || right (255 bits) = 52 words,
    (n, 4) and (n, 4) -> (n, 4).  `domain`: a HashDomain, a name or None for Orchard's.  Raises `Bottom` where the specification's
    hash has no value (Orchard maps that to 0; a caller who wants that catches it)."""
    import torch
    dom = _merkle_domain(domain)
    host = not _is_torch(left)
    dev = fields.current_device()
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)) if host else (lambda a: a)
    l, r = up(left), up(right)
    if l.shape != r.shape or l.ndim != 2 or l.shape[1] != 4 or l.dtype != torch.int64:
        raise ValueError("sinsemilla.merkle_crh: left and right are (n, 4) arrays of Montgomery limbs")
    out = _merkle_layer(dom, layer, torch.stack((l, r), dim=1).contiguous())
    return out.cpu().numpy().view(np.uint64) if host else out


def _merkle_layer(dom, layer, pairs):
    """pairs: (n, 2, 4) int64 CUDA tensor -> (n, 4)"""
    import torch
    if not 0 <= layer < 1 << K:
        raise ValueError("sinsemilla.merkle_crh: the layer is a 10-bit number")
    n = pairs.shape[0]
    tab = _device_table(dom.table)
    out = torch.empty((n, 4), dtype=torch.int64, device=pairs.device)
    status = torch.empty((n,), dtype=torch.uint8, device=pairs.device)
    check(lib().h2_sinsemilla_merkle_layer_device(layer, _ptr(pairs), n, _p(_q_limbs(dom.Q)), tab.data_ptr(), _ptr(out), _ptr(status),
                                                  _stream_ptr()), "h2_sinsemilla_merkle_layer_device")
    _raise_bottom(status, "sinsemilla.merkle_crh")
    return out


def merkle_root(leaves, domain=None):
    """The root of the binary tree over a power-of-two number of leaves, (n, 4) -> (4,): one launch per layer, every layer stays on
    the device.  The tree has depth log2(n) and level l counted from the leaves is hashed with layer = depth - 1 - l, as Orchard
    numbers them (the root's children meet at layer 0).  Any other number of leaves is rejected."""
    import torch
    dom = _merkle_domain(domain)
    host = not _is_torch(leaves)
    t = torch.from_numpy(np.ascontiguousarray(leaves, dtype=np.uint64).view(np.int64)).to(fields.current_device()) if host else leaves.contiguous()
    n = t.shape[0] if t.ndim == 2 else 0
    if t.ndim != 2 or t.shape[1] != 4 or n < 1 or n & (n - 1):
        raise ValueError("sinsemilla.merkle_root: a power-of-two number of leaves, (n, 4) Montgomery limbs")
    depth = n.bit_length() - 1
    for level in range(depth):
        t = _merkle_layer(dom, depth - 1 - level, t.view(t.shape[0] // 2, 2, 4))
    return t[0].cpu().numpy().view(np.uint64) if host else t[0]


MAX_MERKLE_DEPTH = 32                           # the reference's leaf_pos is a u32
MERKLE_PIECE_WORDS = (25, 2, 25)                # the pieces a, b, c of MerkleChip.hash_layer


def _paths_descriptor(dom, depth):
    """-> (h2_merkle_paths_t on the current stream, what it points to: kept alive by the caller until the call has returned).
    dom = None: a descriptor without Q and table, which the trace does not read."""
    from ._lib import MerklePaths
    if dom is None:
        return MerklePaths(depth, None, None, _stream_ptr().value), None
    q, tab = _q_limbs(dom.Q), _device_table(dom.table)
    return MerklePaths(depth, q.ctypes.data_as(C.POINTER(C.c_uint64)), tab.data_ptr(), _stream_ptr().value), (q, tab)


def _path_inputs(what, first, positions, siblings, width):
    """The three arrays of a path call, all of the kind of `first` -> (first (n, width, 4) or (n, 4), positions (n,) int32, siblings
    (n, depth, 4)) as CUDA tensors, and whether they came from the host"""
    import torch
    host = not _is_torch(first)
    if host == _is_torch(siblings) or host == _is_torch(positions):
        raise ValueError(f"{what}: every argument of one kind, numpy arrays or CUDA tensors")
    dev = fields.current_device()
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)) if host else (lambda a: a.contiguous())
    f, s = up(first), up(siblings)
    if host:
        pos = np.asarray(positions)
        if pos.ndim != 1 or (pos.size and (int(pos.min()) < 0 or int(pos.max()) >= 1 << 32)):
            raise ValueError(f"{what}: positions are n numbers below 2^32")
        pos = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.uint32).view(np.int32)).to(dev)
    else:
        pos = positions.contiguous()
    n = pos.shape[0] if pos.ndim == 1 else -1
    if s.ndim != 3 or s.shape[0] != n or s.shape[2] != 4 or not 1 <= s.shape[1] <= MAX_MERKLE_DEPTH or s.dtype != torch.int64 or not s.is_cuda:
        raise ValueError(f"{what}: siblings is an (n, depth, 4) array of Montgomery limbs, depth 1 .. 32")
    depth = s.shape[1]
    if tuple(f.shape) != ((n, 4) if width is None else (n, depth + width, 4)) or f.dtype != torch.int64 or not f.is_cuda:
        raise ValueError(f"{what}: " + ("leaves is (n, 4)" if width is None else "nodes is (n, depth + 1, 4)") + " Montgomery limbs")
    if pos.dtype != torch.int32 or not pos.is_cuda:
        raise ValueError(f"{what}: positions is an (n,) array of uint32 (a CUDA int32 tensor holds their bits)")
    return f, pos, s, host


def merkle_paths(leaves, positions, siblings, domain=None, with_status: bool = False):
    """The walk of n Merkle paths (merkle.rs MerklePath::calculate_root) in ONE launch, one lane per path: leaves (n, 4), positions
    (n,) and siblings (n, depth, 4) -> nodes (n, depth + 1, 4): node 0 is the leaf, node l + 1 = MerkleCRH(l, left, right) with
    (left, right) = (sibling_l, node_l) where bit l of the position is set, (node_l, sibling_l) where it is not; node `depth` is the
    root.  Host arrays (positions any integer type below 2^32) or CUDA tensors (positions an int32 tensor holding the u32 bits), with
    the conventions of `merkle_crh`.  A layer without a value raises `Bottom`; with_status: returns (nodes, status (n, depth) uint8)
    instead, the node of such a layer 0 and the walk continued from it."""
    import torch
    dom = _merkle_domain(domain)
    lv, pos, sib, host = _path_inputs("sinsemilla.merkle_paths", leaves, positions, siblings, None)
    n, depth = sib.shape[0], sib.shape[1]
    nodes = torch.empty((n, depth + 1, 4), dtype=torch.int64, device=sib.device)
    status = torch.empty((n, depth), dtype=torch.uint8, device=sib.device)
    d, keep = _paths_descriptor(dom, depth)
    check(lib().h2_sinsemilla_merkle_paths_device(C.byref(d), _ptr(lv), _ptr(sib), _ptr(pos), n, _ptr(nodes), _ptr(status)),
          "h2_sinsemilla_merkle_paths_device")
    del keep
    if with_status:
        return (nodes.cpu().numpy().view(np.uint64), status.cpu().numpy()) if host else (nodes, status)
    _raise_bottom(status, "sinsemilla.merkle_paths")
    return nodes.cpu().numpy().view(np.uint64) if host else nodes


class MerklePathTrace:
    """What `merkle_path_trace` returns: views of the one buffer h2_sinsemilla_merkle_trace_device writes (include/halo2_mi355x.h), each
    a whole column vector.  With count = n * (layer_hi - layer_lo) items, item t = path * layers + (l - layer_lo):
        swap_rows   (5, count, 4)      a (node), b (sibling), a_swapped (left), b_swapped (right), swap
        pieces      (3 * count, 4)     a, b, c of item t at 3 t .., Montgomery: the witness_pieces column
        decompose   (5, 2 * count, 4)  the rows of "Check piece decomposition", advice columns 0 .. 4
        canonical   (count, 3, 4)      the pieces as CANONICAL limbs: `trace`'s pieces
        b_1, b_2    (count, 4)         CANONICAL: the values of the two 5-bit range checks"""

    def __init__(self, out, n, layers):
        self.out, self.n, self.layers, c = out, n, layers, n * layers
        self.count = c
        self.swap_rows = out[:5 * c].reshape(5, c, 4)
        self.pieces = out[5 * c:8 * c]
        self.decompose = out[8 * c:18 * c].reshape(5, 2 * c, 4)
        self.canonical = out[18 * c:21 * c].reshape(c, 3, 4)
        self.b_1, self.b_2 = out[21 * c:22 * c], out[22 * c:23 * c]


def merkle_path_trace(nodes, positions, siblings, layer_lo: int, layer_hi: int, domain=None) -> MerklePathTrace:
    """The cells MerkleChip.hash_layer and CondSwapChip.swap assign outside the hash region, for the layers [layer_lo, layer_hi) of
    every path: nodes (n, depth + 1, 4) as `merkle_paths` returns them, positions and siblings as it takes them.  The 53-row chains
    come from `trace(result.canonical, MERKLE_PIECE_WORDS, Q)`.  `domain` is accepted for symmetry; no cell here depends on it."""
    import torch
    nd, pos, sib, host = _path_inputs("sinsemilla.merkle_path_trace", nodes, positions, siblings, 1)
    n, depth = sib.shape[0], sib.shape[1]
    layer_lo, layer_hi = int(layer_lo), int(layer_hi)
    if not 0 <= layer_lo < layer_hi <= depth:
        raise ValueError("sinsemilla.merkle_path_trace: 0 <= layer_lo < layer_hi <= depth")
    layers = layer_hi - layer_lo
    out = torch.empty((23 * n * layers, 4), dtype=torch.int64, device=sib.device)
    d, keep = _paths_descriptor(None, depth)
    check(lib().h2_sinsemilla_merkle_trace_device(C.byref(d), _ptr(nd), _ptr(sib), _ptr(pos), n, layer_lo, layer_hi, _ptr(out)),
          "h2_sinsemilla_merkle_trace_device")
    del keep
    return MerklePathTrace(out.cpu().numpy().view(np.uint64) if host else out, n, layers)


def _trace(name, entry, lead, pieces, num_words, q_of, table, with_status):
    """What `trace` (lead = 0) and `trace_from` (lead = 1 more row per message) share: the checks of pieces and num_words, the call of
    lib().<entry> and the status.  q_of(p, count, host) -> the entry point's Q argument, a host pointer or a CUDA tensor."""
    import torch
    num_words = [int(w) for w in num_words]
    host = not _is_torch(pieces)
    p = torch.from_numpy(np.ascontiguousarray(pieces, dtype=np.uint64).view(np.int64)).to(fields.current_device()) if host else pieces.contiguous()
    if p.ndim != 3 or p.shape[1] != len(num_words) or p.shape[2] != 4 or p.dtype != torch.int64:
        raise ValueError(f"sinsemilla.{name}: pieces is a (count, n_pieces, 4) array of canonical limbs")
    if not num_words or any(not 1 <= w <= 25 for w in num_words) or sum(num_words) > C_MAX:
        raise ValueError(f"sinsemilla.{name}: 1 .. 25 words per piece, 253 per message")
    count, rows = p.shape[0], sum(num_words) + 1 + lead
    q = q_of(p, count, host)
    tab = _device_table(table)
    out = torch.empty((5, rows * count, 4), dtype=torch.int64, device=p.device)
    status = torch.empty((count,), dtype=torch.uint8, device=p.device)
    nw = (C.c_uint32 * len(num_words))(*num_words)
    check(getattr(lib(), entry)(_ptr(p), count, nw, len(num_words), _ptr(q) if _is_torch(q) else q, tab.data_ptr(), _ptr(out), _ptr(status),
                                _stream_ptr()), entry)
    if with_status:
        return (out.cpu().numpy().view(np.uint64), status.cpu().numpy()) if host else (out, status)
    _raise_bottom(status, f"sinsemilla.{name}")
    return out.cpu().numpy().view(np.uint64) if host else out


def trace(pieces, num_words, Q, table=None, with_status: bool = False):
    """What SinsemillaChip.hash_to_point witnesses for `count` messages of one piece structure.  pieces: (count, n_pieces, 4) CANONICAL
    limbs (piece k carries num_words[k] <= 25 words, low bits first); Q an (x, y) pair.  -> (5, rows * count, 4) Montgomery limbs, the
    columns x_a, x_p, bits, lambda_1, lambda_2 with rows = sum(num_words) + 1 per message (see include/halo2_mi355x.h).  A message
    without a value raises `Bottom`, or is flagged in the returned status with with_status."""
    return _trace("trace", "h2_sinsemilla_trace_device", 0, pieces, num_words, lambda p, count, host: _p(_q_limbs(Q)), table, with_status)


def trace_from(pieces, num_words, Q, table=None, with_status: bool = False):
    """`trace` for messages that start from a cell: what hash_message_with_private_init witnesses, and a hash from a public Q on a chip
    configured with allow_init_from_private_point (hash_to_point.rs:117-121, :179-182).  Q: (count, 8) Montgomery affine points of the
    kind of `pieces`, or one (x, y) pair of integers for all.  -> (5, rows * count, 4) with rows = sum(num_words) + 2: row 0 of a
    message holds y_Q in x_p and zeros elsewhere, the rest are the rows of `trace` from that Q."""
    def q_of(p, count, host):
        if isinstance(Q, (tuple, list)) and len(Q) == 2 and all(isinstance(c, int) for c in Q):
            import torch
            return torch.from_numpy(_q_limbs(Q).view(np.int64)).to(p.device).repeat(count, 1)
        return _device_points(Q, count, host, "sinsemilla.trace_from")
    return _trace("trace_from", "h2_sinsemilla_trace_from_device", 1, pieces, num_words, q_of, table, with_status)


class CommitDomain:
    """`CommitDomain::new(name)` (the `sinsemilla` crate): M = HashDomain(name + "-M") and R = hash_to_curve(name + "-r")(""), the
    personalisation being the domain string itself.  `fixed_base` is R's `ecc.FixedBase` of 85 windows, built on first use; it is
    what the gadget's `FixedBaseTables.of` takes."""

    def __init__(self, name, table=None):
        from .commitment import hash_to_curve
        name = name.decode() if isinstance(name, bytes) else str(name)
        self.M = HashDomain(name + "-M", table=table)
        self._r_limbs = hash_to_curve(PALLAS, name + "-r", [b""])[0]
        self.R = _points_to_ints(self._r_limbs)[0]
        self._fixed_base = None

    @property
    def fixed_base(self):
        if self._fixed_base is None:
            from . import ecc
            self._fixed_base = ecc.FixedBase(self._r_limbs, ecc.NUM_WINDOWS)
        return self._fixed_base

    def commit(self, words, r, with_status: bool = False, Q=None):
        """SinsemillaHashToPoint(Q, words_i) + [r_i]R for n messages: words as `HashDomain.hash_to_point`, r (n, 4) CANONICAL limbs read
        as `ecc.mul_fixed` reads them, Q as `hash_to_point` -> (n, 8).  The sum is the group's, so it may be the identity, (0, 0); only
        a HASH without a value raises `Bottom`, or is flagged in the returned status with with_status."""
        import torch
        w, host = _device_words(words, "sinsemilla.commit")
        n, length = w.shape
        k = _device_limbs(r, n, 4, host, "sinsemilla.commit r")
        q = None if Q is None else _device_points(Q, n, host, "sinsemilla.commit")
        tab = _device_table(self.M.table)
        out = torch.empty((n, 8), dtype=torch.int64, device=w.device)
        status = torch.empty((n,), dtype=torch.uint8, device=w.device)
        check(lib().h2_sinsemilla_commit_device(_ptr(w), n, length, _p(_q_limbs(self.M.Q)) if q is None else None,
                                                None if q is None else q.data_ptr(), tab.data_ptr(), self.fixed_base.points.data_ptr(),
                                                _ptr(k), _ptr(out), _ptr(status), _stream_ptr()), "h2_sinsemilla_commit_device")
        if with_status:
            return (out.cpu().numpy().view(np.uint64), status.cpu().numpy()) if host else (out, status)
        _raise_bottom(status, "sinsemilla.commit")
        return out.cpu().numpy().view(np.uint64) if host else out

    def short_commit(self, words, r, with_status: bool = False, Q=None):
        """The x coordinates of `commit`, 0 for the identity (extract_p): -> (n, 4)."""
        res = self.commit(words, r, with_status, Q)
        pts = res[0] if with_status else res
        xs = np.ascontiguousarray(pts[:, :4]) if isinstance(pts, np.ndarray) else pts[:, :4].contiguous()
        return (xs, res[1]) if with_status else xs
