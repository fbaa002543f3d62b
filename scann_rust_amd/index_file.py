"""numpy reader / writer of the SCANNIDX index container (include/scann_hip.h "index files").

The same bytes scann_hip_txh_write_file / scann_hip_index_load_file handle, so that the CPU oracle,
the golden fixtures and any offline tool can share index files with the GPU library without going
through it.  Arrays come back as read-only np.memmap views (nothing is copied).
"""
import struct

import numpy as np

MAGIC = b"SCANNIDX"
VERSION = 1
ALIGN = 4096
_DTYPES = {0: np.float32, 1: np.uint32, 2: np.uint8}
_CODES = {np.dtype(np.float32): 0, np.dtype(np.uint32): 1, np.dtype(np.uint8): 2}
_ROWS_Q_DTYPES = {1: np.uint16, 2: np.uint8, 3: np.int8}   # SCANN_HIP_ROWS_BF16 / _FP8_E4M3 / _INT8
# magic, version, kind, n_rows, n_local, file_bytes, dim, stride, L, S, K, dsub, measure, csr, packed4,
# residuals, partitions_to_search, multiplier, n_sections
_HEADER = struct.Struct("<8sIIQQQIIIIIIiiiiIfI")
_SECTION = struct.Struct("<24sIIQQ16x")
_FIELDS = ["version", "kind", "n_rows", "n_local", "file_bytes", "dim", "stride", "num_partitions",
           "num_subspaces", "num_codes", "dims_per_subspace", "distance_measure", "data_is_csr_order",
           "codes_packed4", "use_residuals", "partitions_to_search", "pre_reorder_multiplier", "n_sections"]


def read(path):
    """-> (header dict, {section name: np.memmap})."""
    with open(path, "rb") as f:
        raw = f.read(256)
        if len(raw) < 256:
            raise ValueError("DataLoss: %s is shorter than an index header" % path)
        vals = _HEADER.unpack_from(raw)
        if vals[0] != MAGIC:
            raise ValueError("InvalidArgument: %s is not a SCANNIDX file" % path)
        header = dict(zip(_FIELDS, vals[1:]))
        if header["version"] != VERSION:
            raise ValueError("InvalidArgument: unsupported index file version %d" % header["version"])
        table = f.read(64 * header["n_sections"])
        f.seek(0, 2)
        if f.tell() != header["file_bytes"]:
            raise ValueError("DataLoss: %s is %d bytes, header says %d" % (path, f.tell(), header["file_bytes"]))
    sections = {}
    for i in range(header["n_sections"]):
        name, dtype, _, off, nbytes = _SECTION.unpack_from(table, 64 * i)
        dt = np.dtype(_DTYPES[dtype])
        if off % ALIGN or off + nbytes > header["file_bytes"] or nbytes % dt.itemsize:
            raise ValueError("DataLoss: section table out of bounds")
        sections[name.rstrip(b"\0").decode()] = np.memmap(path, dt, "r", off, (nbytes // dt.itemsize,)) \
            if nbytes else np.empty(0, dt)
    return header, sections


def arrays(path):
    """The file's arrays in their natural shapes: the keyword arguments of hip.txh_create /
    the CPU checker's index view (kind 1) or (data, n, dim, stride, measure) pieces (kind 0)."""
    h, s = read(path)
    out = dict(h)
    if "proj_meta" in s:   # a projected handle (hip.txh_create_projected): "data" holds the original rows at row_stride
        kind, in_dim, out_dim, start, row_stride = (int(v) for v in s["proj_meta"][:5])
        out["proj_meta"] = s["proj_meta"]
        out["projection"] = dict(kind=kind, in_dim=in_dim, out_dim=out_dim, start=start, row_stride=row_stride)
        if "proj_matrix" in s:
            out["proj_matrix"] = s["proj_matrix"].reshape(out_dim, in_dim)
        if "proj_mean" in s:
            out["proj_mean"] = s["proj_mean"]
        if "data" in s:
            out["data"] = s["data"].reshape(h["n_rows"], row_stride)
    elif "data" in s:
        out["data"] = s["data"].reshape(h["n_rows"], h["stride"])
    if "rows_q" in s:   # a handle over quantized rows (hip.txh_create_quantized): no "data"
        fmt = int(s["rows_q_meta"][0])
        out["rows_q_meta"] = s["rows_q_meta"]
        out["fmt"] = fmt
        out["inv_multiplier"] = float(np.asarray(s["rows_q_meta"][1:2]).view(np.float32)[0])
        out["rows_q"] = s["rows_q"].view(_ROWS_Q_DTYPES[fmt]).reshape(h["n_rows"], h["stride"])
    if h["kind"] == 1:
        if h["num_partitions"]:
            out["centers"] = s["centers"].reshape(h["num_partitions"], h["dim"])
            out["leaf_offsets"] = s["leaf_offsets"]
            out["leaf_ids"] = s["leaf_ids"]
            if "leaf_sizes_global" in s:
                out["leaf_sizes_global"] = s["leaf_sizes_global"]
        if h["num_subspaces"]:
            out["codebook"] = s["codebook"].reshape(h["num_subspaces"], h["num_codes"], h["dims_per_subspace"])
            bpp = (h["num_subspaces"] + 1) // 2 if h["codes_packed4"] else h["num_subspaces"]
            out["codes"] = s["codes"].reshape(h["n_local"], bpp)
    return out


def rows_q_sections(rows, fmt, inv_multiplier=1.0):
    """The two sections of quantized re-rank rows for write(): the rows' bytes and {format, inv_multiplier bits}."""
    r = np.ascontiguousarray(rows).view(_ROWS_Q_DTYPES[fmt])
    meta = np.array([fmt, np.array([inv_multiplier], np.float32).view(np.uint32)[0]], np.uint32)
    return [("rows_q", r.reshape(-1).view(np.uint8)), ("rows_q_meta", meta)]


def write(path, *, kind, n_rows, n_local, dim, stride, num_partitions=0, num_subspaces=0, num_codes=0,
          dims_per_subspace=0, distance_measure=0, data_is_csr_order=0, codes_packed4=0, use_residuals=0,
          partitions_to_search=0, pre_reorder_multiplier=0.0, sections=()):
    """sections: ordered (name, array) pairs; dtype f32 / u32 / u8."""
    secs = [(n, np.ascontiguousarray(a)) for n, a in sections]
    off = 256 + 64 * len(secs)
    table = b""
    offsets = []
    for name, a in secs:
        off = (off + ALIGN - 1) // ALIGN * ALIGN
        table += _SECTION.pack(name.encode(), _CODES[a.dtype], 0, off, a.nbytes)
        offsets.append(off)
        off += a.nbytes
    head = _HEADER.pack(MAGIC, VERSION, kind, n_rows, n_local, off, dim, stride, num_partitions, num_subspaces,
                        num_codes, dims_per_subspace, distance_measure, data_is_csr_order, codes_packed4,
                        use_residuals, partitions_to_search, pre_reorder_multiplier, len(secs))
    with open(path, "wb") as f:
        f.write(head.ljust(256, b"\0"))
        f.write(table)
        for (name, a), o in zip(secs, offsets):
            f.write(b"\0" * (o - f.tell()))
            f.write(a.tobytes())
