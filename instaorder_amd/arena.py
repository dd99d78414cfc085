"""The byte layout the device input pipeline shares, and what a codec hands to whoever lays a batch out.
``datasets.PairRenderer.render`` places a whole batch by it; ``rle.decode``, ``poly.decode``, ``jpeg.decode`` and
``png.decode`` place the tables of one call (``decode_into``).

The one rule: every blob starts on a multiple of 16 bytes (the descriptor structs hold int64) and takes its size rounded
up to 16, at least 16 -- an empty blob still gets an address of its own.
"""
import numpy as np


def room(nbytes):
    """the bytes a blob of ``nbytes`` takes"""
    return (max(int(nbytes), 1) + 15) // 16 * 16


class Layout(object):
    """hands out offsets: ``at = lay.add(nbytes)``; ``lay.size`` is the end of what has been handed out"""

    def __init__(self):
        self.size = 0

    def add(self, nbytes):
        at = self.size
        self.size += room(nbytes)
        return at


def pack(blobs, offsets=None, host=None):
    """Writes every uint8 blob at its offset of ``host`` and zeros the padding behind it; returns (host, offsets).  Without
    ``offsets`` the blobs are laid out from 0; without ``host`` they go into a fresh buffer that ends with the last one."""
    if offsets is None:
        lay = Layout()
        offsets = [lay.add(b.size) for b in blobs]
    if host is None:
        host = np.empty(max([a + room(b.size) for a, b in zip(offsets, blobs)] or [0]), np.uint8)
    for a, b in zip(offsets, blobs):
        host[a:a + b.size] = b
        host[a + b.size:a + room(b.size)] = 0
    return host, offsets


def as_bytes(array):
    """the uint8 view of a ctypes array or a NumPy array: it aliases the array, so a field set later shows through it"""
    if isinstance(array, np.ndarray):
        return array.view(np.uint8).reshape(-1)
    return np.frombuffer(array, dtype=np.uint8)


class Group(object):
    """The members of a batch that one library call decodes, as ``rle.group``, ``poly.group``, ``jpeg.group``,
    ``jpeg.group_progressive`` and ``png.group`` build it:

    blobs     the uint8 host views that travel to the device, in a fixed order (``as_bytes`` of the tables)
    classes   per blob "images", "masks" or "descriptors": where ``PairRenderer.last_upload`` counts it
    outs      the descriptor array with one entry per member; the caller sets their ``out_off`` (``set_outs``)
    images    the members that have a status word (JPEG and PNG files), ``raise_for_status(words, images)`` their
              module's reader of the words; ``n_status`` = their number, 0 for masks
    launch(addrs, out, out_bytes, ws, ws_bytes, status, stream, info=None)
              the one call of the entry point; ``addrs``: the device address of every blob, all addresses as ints

    A group without members (the default arguments) has no blobs, no workspace and no status words; ``launch`` is not
    called for it."""

    def __init__(self, blobs=(), classes=(), outs=(), launch=None, workspace_bytes=None, images=(),
                 raise_for_status=None):
        self.blobs, self.classes, self.outs, self.launch = list(blobs), tuple(classes), outs, launch
        self._workspace_bytes, self.images, self.raise_for_status = workspace_bytes, list(images), raise_for_status
        self.n_status = len(self.images)

    def __len__(self):
        return len(self.outs)

    def set_outs(self, offsets):
        for k, o in enumerate(offsets):
            self.outs[k].out_off = int(o)

    def workspace_bytes(self):
        """asked after the out-offsets are set; 0 where the codec has no workspace"""
        return self._workspace_bytes() if self._workspace_bytes else 0


def decode_into(groups, out, status=None, info=None):
    """What the four ``decode()`` functions share: the blobs of ``groups`` in one upload, a workspace per group, and the
    launches in the order given on the current stream of ``out`` (a uint8 device tensor, the arena of the out-offsets).
    ``status`` / ``info``: int32 device tensors with one word per image of the groups, in their order, or None.

    The upload and the workspaces are allocated and consumed on that one stream, so the allocator hands their memory out
    again only behind the launches: no ``record_stream``, here or in the callers."""
    import torch
    groups = [g for g in groups if len(g)]
    if not groups:
        return
    host, ats = pack([b for g in groups for b in g.blobs])
    dev = torch.from_numpy(host).to(out.device)
    stream = torch.cuda.current_stream(out.device).cuda_stream
    first = 0
    for g in groups:
        addrs = [dev.data_ptr() + a for a in ats[:len(g.blobs)]]
        ats = ats[len(g.blobs):]
        ws = torch.empty(g.workspace_bytes(), dtype=torch.uint8, device=out.device)
        g.launch(addrs, out.data_ptr(), out.numel(), ws.data_ptr(), ws.numel(),
                 status.data_ptr() + 4 * first if g.n_status else 0, stream,
                 info=info.data_ptr() + 4 * first if info is not None else None)
        first += g.n_status
