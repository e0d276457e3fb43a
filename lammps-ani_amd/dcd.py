"""A DCD trajectory writer in pure Python: the little-endian CHARMM / NAMD file that LAMMPS' ``dump dcd`` writes, for the frames of
``VerletRun.set_dump`` (md.py), whose device layout -- all x, then all y, then all z, fp32 -- is the file's own.

Header, 276 bytes, every record between two int32 byte counts:
  1. 84 bytes: "CORD", int32 NSET (frames in the file, at file offset 8), int32 first step, int32 steps between frames, int32 last
     step (file offset 20), five int32 zeros, float32 dt, int32 1 (a unit cell comes with every frame), eight int32 zeros, int32 24
  2. 164 bytes: int32 2 and two remark lines of 80 characters, space-padded
  3. 4 bytes: int32 natoms
A frame, 56 + 3 (4 N + 8) bytes: a record of six float64 [len_x, 0, len_y, 0, 0, len_z] (the zeros are the angle cosines of an
orthogonal box), then one record of N float32 for each of x, y, z.  NSET and the last step are rewritten after every frame, so a file
is readable whenever the writer is between two appends.
"""
from __future__ import annotations

import struct

HEADER_BYTES = 276
REMARKS = ("REMARKS trajectory of the lammps-ani_amd timestep loop", "REMARKS atoms in ascending order of their global tag")


def frame_bytes(natoms: int) -> int:
    return 56 + 3 * (4 * int(natoms) + 8)


class DCDWriter:
    def __init__(self, path, natoms: int, first_step: int, every: int, dt: float):
        """path: created or truncated; natoms per frame; first_step: the step of the first frame; every: steps between two
        frames; dt: the timestep, as LAMMPS writes it (fs under ``units real``)."""
        if int(natoms) < 1 or int(every) < 1:
            raise ValueError("DCDWriter: natoms >= 1 and every >= 1")
        self.path, self.natoms, self.first_step, self.every, self.dt = str(path), int(natoms), int(first_step), int(every), float(dt)
        self.nframes = 0
        self._f = open(self.path, "wb")
        rec1 = b"CORD" + struct.pack("<9i", 0, self.first_step, self.every, self.first_step, 0, 0, 0, 0, 0) \
            + struct.pack("<f", self.dt) + struct.pack("<10i", 1, 0, 0, 0, 0, 0, 0, 0, 0, 24)
        rec2 = struct.pack("<i", 2) + b"".join(r.encode("ascii")[:80].ljust(80) for r in REMARKS)
        rec3 = struct.pack("<i", self.natoms)
        for rec in (rec1, rec2, rec3):
            self._f.write(struct.pack("<i", len(rec)) + rec + struct.pack("<i", len(rec)))
        assert self._f.tell() == HEADER_BYTES
        self._f.flush()

    @property
    def last_step(self) -> int:
        return self.first_step + max(self.nframes - 1, 0) * self.every

    def append(self, cell, xyz_block):
        """One frame.  cell: six numbers, lo then len of the box (the `cell` of ani_md_frame_pack), or the three lengths alone;
        xyz_block: the 3 N float32 values of the frame, all x, then all y, then all z -- bytes, or anything with tobytes()
        (a [3, N] float32 array)."""
        if self._f is None:
            raise ValueError("DCDWriter.append: the file is closed")
        cell = [float(c) for c in cell]
        if len(cell) not in (3, 6):
            raise ValueError("DCDWriter.append: cell takes 6 numbers (lo, len) or 3 (len)")
        lx, ly, lz = cell[-3:]
        data = xyz_block if isinstance(xyz_block, (bytes, bytearray, memoryview)) else xyz_block.tobytes()
        n4 = 4 * self.natoms
        if len(data) != 3 * n4:
            raise ValueError(f"DCDWriter.append: a frame of {self.natoms} atoms takes {3 * n4} bytes of float32, got {len(data)}")
        f = self._f
        f.seek(0, 2)
        f.write(struct.pack("<i6di", 48, lx, 0.0, ly, 0.0, 0.0, lz, 48))
        mark = struct.pack("<i", n4)
        for k in range(3):
            f.write(mark)
            f.write(data[k * n4:(k + 1) * n4])
            f.write(mark)
        self.nframes += 1
        f.seek(8)
        f.write(struct.pack("<i", self.nframes))
        f.seek(20)
        f.write(struct.pack("<i", self.last_step))
        f.flush()

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None
