#!/usr/bin/env python3
"""Write the inputs of the reference's example/run.R as fixtures of tests/test_gpu_create_object.py.

  python tests/golden/create_object_example/make_inputs.py <inferCNV checkout>/inst/extdata

The three files are data that CreateInfercnvObject reads.  The gene-position and the annotation file are kept byte for byte
and compressed (read.table reads a compressed file as it reads a plain one, and so do the library and the restatement).
The counts matrix (2.9 MB compressed) is over the size limit of a committed file, so the header line and every eighth gene
row (rows 0, 8, 16, ... of the body) are kept.  Every file is compressed with a zeroed time stamp: the bytes are reproducible.
"""
import gzip
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
MATRIX = "oligodendroglioma_expression_downsampled.counts.matrix.gz"
GENES = "gencode_downsampled.EXAMPLE_ONLY_DONT_REUSE.txt"
ANNOTATIONS = "oligodendroglioma_annotations_downsampled.txt"


def write_gz(name, data):
    with open(os.path.join(HERE, name), "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as out:
            out.write(data)


def main(src):
    for name in (GENES, ANNOTATIONS):
        with open(os.path.join(src, name), "rb") as fh:
            write_gz(name + ".gz", fh.read())
    with gzip.open(os.path.join(src, MATRIX), "rb") as fh:
        lines = fh.read().split(b"\n")
    body = [ln for ln in lines[1:] if ln]
    kept = [lines[0]] + body[::8]
    write_gz("counts_every_8th_gene.matrix.gz", b"\n".join(kept) + b"\n")
    print(f"{len(body)} gene rows, {len(kept) - 1} kept")


if __name__ == "__main__":
    main(sys.argv[1])
