"""Bit-serial CRC-64/NVME, written from the checksum's parameters alone:
width 64, polynomial 0xAD93D23594C93659, input and output reflected, init
and xorout all ones. Independent of csrc/crc64.h (no tables, no reflected
constant copied from it); slow, so it is the oracle for short inputs only.
"""

import base64
import struct

WIDTH = 64
POLY = 0xAD93D23594C93659
MASK = (1 << WIDTH) - 1


def _reflect(v: int, bits: int) -> int:
    out = 0
    for i in range(bits):
        if v >> i & 1:
            out |= 1 << (bits - 1 - i)
    return out


def crc64nvme(data: bytes) -> int:
    """MSB-first shift register over reflected input bytes, reflected out."""
    reg = MASK  # init
    top = 1 << (WIDTH - 1)
    for byte in data:
        reg ^= _reflect(byte, 8) << (WIDTH - 8)
        for _ in range(8):
            reg = ((reg << 1) ^ POLY) & MASK if reg & top else (reg << 1) & MASK
    return _reflect(reg, WIDTH) ^ MASK  # refout, xorout


def header_value(crc: int) -> str:
    """x-amz-checksum-crc64nvme: base64 of the 8 bytes, big-endian."""
    return base64.b64encode(struct.pack(">Q", crc)).decode()
