#!/usr/bin/env python
"""Converts the polygon (and uncompressed-RLE) segmentations of an LVIS / COCO annotation json to compressed COCO RLE,
once, offline: what ``TrainPipeline.prepare`` and ``LVISEval(..., 'segm')`` take.

    python tools/lvis_polygons_to_rle.py IN.json OUT.json [--device cuda:0]

Every annotation's ``'segmentation'`` becomes ``{'size': [h, w], 'counts': str}`` at its image's size
(``LVISGroundTruth.rasterize_polygons``: all polygons of the file in one device batch, csrc/poly_rle.hip); everything
else in the file is written back as it was read.  Needs the GPU.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def convert(dataset, device=None):
    """The loaded json, converted in place; returns the number of annotations converted."""
    from balancedgroupsoftmax_amd.lvis_eval import LVISGroundTruth
    n = LVISGroundTruth(dataset).rasterize_polygons(device)
    for a in dataset['annotations']:
        seg = a.get('segmentation')
        if isinstance(seg, dict) and isinstance(seg['counts'], bytes):
            seg['counts'] = seg['counts'].decode('ascii')                  # (json has no bytes)
    return n


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('src')
    ap.add_argument('dst')
    ap.add_argument('--device', default=None)
    a = ap.parse_args(argv)
    with open(a.src) as f:
        dataset = json.load(f)
    n = convert(dataset, a.device)
    with open(a.dst, 'w') as f:
        json.dump(dataset, f)
    print('%s: %d of %d segmentations converted -> %s' % (a.src, n, len(dataset['annotations']), a.dst))
    return 0


if __name__ == '__main__':
    sys.exit(main())
