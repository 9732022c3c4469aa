"""The class centres of the NCM (nearest-class-mean) baseline: what the reference's DCM detector reads from
``./data/lvis/dcm_center_fea.pt`` (mmdet/models/detectors/DCM.py:38-42) and how that file comes to be.

* ``ClassCenters``   the per-class feature sums and counts, device resident.  The reference's collection epoch
                     (DCM.py:82-105) writes three files per training image and leaves the averaging to a script that
                     is not in its tree; here ``update`` is one launch per batch (``functional.class_sum``: fp64 sums in
                     ascending row order, no atomics) and ``centers()`` the division.
* ``load_centers``   the arithmetic of ``DCM.__init__`` (:39-41): drop row 0, divide every row by its L2 norm in
                     float32 on the CPU (the reference's bits), then move to the device.

Layouts.  The reference flattens its RoI features ``[K, 256, 7, 7]`` channel-major: column ``c * 49 + h * 7 + w``.  This
package's RoI features are ``[K, 7, 7, 256]``: column ``(h * 7 + w) * 256 + c``.  ``layout='chw'`` says that the feature
is such a map: sums, ``centers()`` and the unit centres are kept in THIS package's column order (what the kernels read),
and ``save`` / ``load_centers`` permute once on the host, so the files are the reference's.  ``layout='flat'`` (the FC
feature) has no permutation.
"""
import torch

from . import functional as BF

LAYOUTS = ('chw', 'flat')


def _check_layout(layout, dim, spatial):
    if layout not in LAYOUTS:
        raise ValueError("layout must be 'chw' (a [C, h, w] map, stored channel-major by the reference) or 'flat', "
                         'got %r' % (layout,))
    if layout == 'chw' and (spatial < 1 or dim % spatial != 0):
        raise ValueError("layout 'chw': dim %d is not a multiple of the %d positions of the map" % (dim, spatial))


def to_reference_layout(m, layout, spatial=49):
    """``[N, D]`` in this package's column order -> the reference's (``'chw'``: ``(s, c)`` -> ``(c, s)``)."""
    if layout == 'flat':
        return m
    N, D = m.shape
    return m.view(N, spatial, D // spatial).permute(0, 2, 1).reshape(N, D)


def from_reference_layout(m, layout, spatial=49):
    """The inverse of :func:`to_reference_layout`."""
    if layout == 'flat':
        return m
    N, D = m.shape
    return m.view(N, D // spatial, spatial).permute(0, 2, 1).reshape(N, D)


class ClassCenters(object):
    """Running per-class sums of a feature: ``sums [num_classes, dim]`` float64 and ``counts [num_classes]`` int64 on
    the device of the first ``update`` (class 0, the background, is a row like any other; nothing labels a ground
    truth with it).  ``spatial``: the positions of the map under ``layout='chw'`` (7 x 7)."""

    def __init__(self, num_classes, dim, layout='chw', spatial=49):
        _check_layout(layout, int(dim), int(spatial))
        if num_classes < 1 or dim < 1:
            raise ValueError('ClassCenters: num_classes and dim must be positive')
        self.num_classes, self.dim, self.layout, self.spatial = int(num_classes), int(dim), layout, int(spatial)
        self.sums = None
        self._counts = None

    def _state(self, device):
        if self.sums is None:
            self.sums = torch.zeros((self.num_classes, self.dim), dtype=torch.float64, device=device)
            self._counts = torch.zeros((self.num_classes,), dtype=torch.int64, device=device)
        return self.sums, self._counts

    def update(self, fea, labels):
        """``fea [G, ...]`` (flattened to ``[G, dim]`` as it lies in memory) float32 on the GPU, ``labels [G]``: adds
        every row to its class.  No host read; rows labelled outside ``[0, num_classes)`` are skipped."""
        BF._require_cuda(fea, labels)
        fea = fea.detach()
        if fea.dim() < 2 or fea[0].numel() != self.dim:
            raise ValueError('ClassCenters.update: fea %s does not hold rows of %d values'
                             % (tuple(fea.shape), self.dim))
        fea = fea.reshape(fea.shape[0], self.dim).contiguous()
        labels = labels.reshape(-1).to(torch.int64).contiguous()
        if labels.numel() != fea.shape[0]:
            raise ValueError('ClassCenters.update: %d rows, %d labels' % (fea.shape[0], labels.numel()))
        sums, counts = self._state(fea.device)
        step = BF.class_sum_max_rows()
        for g0 in range(0, fea.shape[0], step):      # pieces in row order keep the order of the adds
            BF.class_sum(fea[g0:g0 + step], labels[g0:g0 + step], sums, counts)
        return self

    def counts(self):
        """``[num_classes]`` int64 (zeros before the first update, on the CPU then)."""
        if self._counts is None:
            return torch.zeros((self.num_classes,), dtype=torch.int64)
        return self._counts

    def centers(self):
        """``sum / count`` divided in float64 and rounded once -> float32 ``[num_classes, dim]`` in this package's
        column order; a class that was never seen has a zero row."""
        if self.sums is None:
            return torch.zeros((self.num_classes, self.dim), dtype=torch.float32)
        n = self._counts.to(torch.float64)[:, None]
        return torch.where(n > 0, self.sums / n.clamp(min=1.0), torch.zeros_like(self.sums)).to(torch.float32)

    def save(self, path):
        """Writes ``centers()`` as the file the reference loads: float32 ``[num_classes, dim]`` on the CPU, columns in
        the REFERENCE's order."""
        torch.save(to_reference_layout(self.centers().cpu(), self.layout, self.spatial).contiguous(), path)
        return path


def load_centers(path, layout='chw', spatial=49, device=None, expect=None):
    """``DCM.__init__`` (DCM.py:39-41) on a centres file in the reference's layout: row 0 dropped, every row divided by
    its L2 norm (float32 torch on the CPU, so the bits are the reference's ``self.centers``), then the columns brought
    into this package's order -> ``[num_classes - 1, dim]`` float32 on ``device``.

    A class whose centre has norm 0 (never collected) makes the reference's division 0 / 0: every score of every
    proposal becomes NaN through the softmax.  Here that is a ``ValueError`` naming the classes.
    ``expect``: the ``(num_classes, dim)`` the file must have (``ValueError`` otherwise)."""
    centers = torch.as_tensor(torch.load(path, map_location='cpu'))
    if centers.dim() != 2 or centers.shape[0] < 2 or centers.dtype != torch.float32:
        raise ValueError('%s: expected a float32 [num_classes, dim] matrix, got %s %s'
                         % (path, centers.dtype, tuple(centers.shape)))
    if expect is not None and tuple(centers.shape) != tuple(expect):
        raise ValueError('%s holds %d centres of width %d; %d of width %d are needed'
                         % ((path,) + tuple(centers.shape) + tuple(expect)))
    _check_layout(layout, int(centers.shape[1]), int(spatial))
    centers = centers[1:, :]
    norm = centers.norm(dim=1, keepdim=True)
    zero = (torch.nonzero(norm.reshape(-1) == 0).reshape(-1) + 1).tolist()
    if zero:
        raise ValueError('%s: the centre of class%s %s has norm 0 (no feature was collected for it); the NCM scores '
                         'of every proposal would be NaN' % (path, 'es' if len(zero) > 1 else '',
                                                             ', '.join(str(c) for c in zero[:20])
                                                             + (' ...' if len(zero) > 20 else '')))
    unit = from_reference_layout(centers / norm, layout, spatial).contiguous()
    return unit if device is None else unit.to(device)
