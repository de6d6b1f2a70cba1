"""Independent RBF1 writer: pure Python struct + zlib, written from the reference's BruteForceRabitqIndex::save_to_writer
(src/brute_force.rs:305-386)."""
import struct
import zlib

FACTORS = ("delta", "vl", "f_add", "f_rescale", "f_error", "residual_norm", "f_add_ex", "f_rescale_ex")


def write_rbf1(dim, padded_dim, metric, rotator, ex_bits, rotator_blob, bin_codes, ex_codes, factors):
    """bin_codes [n][D/8] u8, ex_codes [n][ex_len] u8 (whatever the index holds: D/8 zero bytes for a trained 1-bit index),
    factors: dict name -> f32 [n]"""
    body = struct.pack("<IIBBBBQQ", dim, padded_dim, metric, rotator, ex_bits, ex_bits + 1, bin_codes.shape[0], len(rotator_blob))
    body += bytes(rotator_blob)
    parts = [body]
    for v in range(bin_codes.shape[0]):
        parts.append(bin_codes[v].tobytes())
        parts.append(ex_codes[v].tobytes())
        parts.append(struct.pack("<8f", *(float(factors[f][v]) for f in FACTORS)))
    body = b"".join(parts)
    return b"RBF1" + struct.pack("<I", 1) + body + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF)
