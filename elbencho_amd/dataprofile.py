"""--dataprofile: merging and reading the profiles that READ phases collect.

The engine (csrc/dataprofile.h) delivers, per worker, a dict of exact
counters, a byte-value histogram and the 16384 registers of a HyperLogLog
sketch. Registers merge by max, everything else by sum, so a profile does not
depend on how the blocks were spread over workers, services or ranks. The
figures a user reads (distinct estimate, dedupe ratio, entropy, suggested
--dedupepct / --compresspct) are derived here and nowhere else.
"""

from __future__ import annotations

import base64
import math
from dataclasses import dataclass, field
from typing import Any

HLL_P = 14
HLL_M = 1 << HLL_P
HLL_ALPHA = 0.7213 / (1 + 1.079 / HLL_M)
_EMPTY_REGS = bytes(HLL_M)


@dataclass
class DataProfile:
    chunks: int = 0
    bytes: int = 0
    zero_chunks: int = 0
    hist: list[int] = field(default_factory=lambda: [0] * 256)
    regs: bytes = _EMPTY_REGS

    # ---- construction / transport ----

    @classmethod
    def from_engine(cls, d: dict[str, Any]) -> "DataProfile":
        """From the dict a worker result carries (regs as bytes)."""
        regs = bytes(d["regs"])
        hist = [int(v) for v in d["hist"]]
        if len(regs) != HLL_M or len(hist) != 256:
            raise ValueError("malformed data profile")
        return cls(int(d["chunks"]), int(d["bytes"]), int(d["zero_chunks"]), hist, regs)

    def to_engine(self) -> dict[str, Any]:
        return {"chunks": self.chunks, "bytes": self.bytes, "zero_chunks": self.zero_chunks,
                "hist": list(self.hist), "regs": self.regs}

    def to_wire(self) -> dict[str, Any]:
        """JSON-safe form for the service protocol (registers as base64)."""
        return {"chunks": self.chunks, "bytes": self.bytes, "zeroChunks": self.zero_chunks,
                "hist": list(self.hist),
                "registers": base64.b64encode(self.regs).decode("ascii")}

    @classmethod
    def from_wire(cls, d: dict[str, Any]) -> "DataProfile":
        return cls.from_engine({"chunks": d["chunks"], "bytes": d["bytes"],
                                "zero_chunks": d["zeroChunks"], "hist": d["hist"],
                                "regs": base64.b64decode(d["registers"])})

    def merge(self, other: "DataProfile") -> "DataProfile":
        """Add other into self (max for the sketch, sum for the rest)."""
        self.chunks += other.chunks
        self.bytes += other.bytes
        self.zero_chunks += other.zero_chunks
        self.hist = [a + b for a, b in zip(self.hist, other.hist)]
        self.regs = bytes(map(max, self.regs, other.regs))
        return self

    # ---- derived figures ----

    def distinct_estimate(self) -> float:
        """HyperLogLog estimate of the number of distinct chunks: the raw
        estimate, replaced by linear counting while it is at most 2.5 m and
        some register is still zero. No large-range correction (64-bit hash)."""
        if not self.chunks:
            return 0.0
        counts = [0] * 64
        for r in self.regs:
            counts[r] += 1
        inv_sum = sum(c * 2.0 ** -r for r, c in enumerate(counts) if c)
        est = HLL_ALPHA * HLL_M * HLL_M / inv_sum
        zeros = counts[0]
        if est <= 2.5 * HLL_M and zeros > 0:
            est = HLL_M * math.log(HLL_M / zeros)
        return est

    def dedupe_ratio(self) -> float:
        est = self.distinct_estimate()
        return self.chunks / est if est > 0 else 0.0

    def entropy_bits_per_byte(self) -> float:
        if not self.bytes:
            return 0.0
        total = float(self.bytes)
        return -sum((c / total) * math.log2(c / total) for c in self.hist if c)

    def compress_bound(self) -> float:
        """8 / entropy: what an order-0 coder could reach (inf for constant data)."""
        ent = self.entropy_bits_per_byte()
        return 8.0 / ent if ent > 0 else math.inf

    def suggest(self) -> dict[str, int]:
        """The nearest --dedupepct / --compresspct that replay this data set."""
        if not self.chunks or not self.bytes:
            return {"dedupepct": 0, "compresspct": 0}
        clamp = lambda v: max(0, min(100, int(v)))  # noqa: E731
        return {
            "dedupepct": clamp(round(100 * (1 - self.distinct_estimate() / self.chunks))),
            "compresspct": clamp(round(100 * self.hist[0] / self.bytes)),
        }

    def to_json(self, chunk_size: int) -> dict[str, Any]:
        """The `dataProfile` object of a phase's JSON result."""
        bound = self.compress_bound()
        return {
            "chunkSize": chunk_size,
            "chunks": self.chunks,
            "bytes": self.bytes,
            "distinctEstimate": round(self.distinct_estimate(), 1),
            "dedupeRatio": round(self.dedupe_ratio(), 4),
            "zeroChunks": self.zero_chunks,
            "zeroBytes": self.hist[0],
            "entropyBitsPerByte": round(self.entropy_bits_per_byte(), 4),
            # JSON has no infinity: constant data reports null
            "compressBound": round(bound, 4) if math.isfinite(bound) else None,
            "suggest": self.suggest(),
            "byteHistogram": list(self.hist),
            "registers": base64.b64encode(self.regs).decode("ascii"),
        }

    def console_lines(self, chunk_size: int) -> list[tuple[str, str]]:
        """(label, value) rows of the console block."""
        bound = self.compress_bound()
        sug = self.suggest()
        zero_share = 100.0 * self.hist[0] / self.bytes if self.bytes else 0.0
        return [
            ("Chunk size", str(chunk_size)),
            ("Chunks total", str(self.chunks)),
            ("Chunks distinct", f"~{self.distinct_estimate():.0f}"),
            ("Dedupe ratio", f"{self.dedupe_ratio():.2f}"),
            ("Chunks zero", str(self.zero_chunks)),
            ("Zero bytes %", f"{zero_share:.1f}"),
            ("Entropy bit/B", f"{self.entropy_bits_per_byte():.3f}"),
            ("Compress bound", f"{bound:.2f}" if math.isfinite(bound) else "inf"),
            ("Replay with", f"--dedupepct {sug['dedupepct']} --compresspct "
                            f"{sug['compresspct']} --dedupechunk {chunk_size}"),
        ]


def merge_profiles(profiles) -> DataProfile | None:
    """Merge an iterable of DataProfile / None; None when there is none."""
    out = None
    for p in profiles:
        if p is None:
            continue
        if out is None:
            out = DataProfile()
        out.merge(p)
    return out
