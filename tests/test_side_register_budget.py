"""The register and LDS budget of the side stream's kernels beside the Schur strips, read from the built code object.

k_schur_window keeps two workgroups on a CU: one wave of each on every SIMD.  A side-stream wave can be placed beside them only in what they leave of
the SIMD's 512 registers (allocated in granules of 8) and of the CU's 160 KiB of LDS.  Only the kernel descriptors' metadata is read (the msgpack note of
the gfx950 code object in libobvi_ba.so: .vgpr_count, .group_segment_fixed_size, .private_segment_fixed_size) -- no instruction text.
"""
import struct

import helpers

SIMD_VGPRS, VGPR_GRANULE, CU_LDS_BYTES = 512, 8, 163840


def _msgpack(buf, pos=0):
    """(value, next position) of the msgpack item at buf[pos] -- the subset the AMDGPU metadata note uses, plus the rest of the scalar types"""
    t = buf[pos]
    pos += 1

    def items(n, pos, pairs):
        out = {} if pairs else []
        for _ in range(n):
            k, pos = _msgpack(buf, pos)
            if pairs:
                v, pos = _msgpack(buf, pos)
                out[k] = v
            else:
                out.append(k)
        return out, pos

    def raw(n, pos, text):
        return (buf[pos:pos + n].decode() if text else bytes(buf[pos:pos + n])), pos + n
    if t <= 0x7f:
        return t, pos
    if t >= 0xe0:
        return t - 0x100, pos
    if 0x80 <= t <= 0x8f:
        return items(t & 0x0f, pos, True)
    if 0x90 <= t <= 0x9f:
        return items(t & 0x0f, pos, False)
    if 0xa0 <= t <= 0xbf:
        return raw(t & 0x1f, pos, True)
    if t == 0xc0:
        return None, pos
    if t in (0xc2, 0xc3):
        return t == 0xc3, pos
    scalars = {0xca: ">f", 0xcb: ">d", 0xcc: ">B", 0xcd: ">H", 0xce: ">I", 0xcf: ">Q", 0xd0: ">b", 0xd1: ">h", 0xd2: ">i", 0xd3: ">q"}
    if t in scalars:
        n = struct.calcsize(scalars[t])
        return struct.unpack(scalars[t], buf[pos:pos + n])[0], pos + n
    lengths = {0xc4: ">B", 0xc5: ">H", 0xc6: ">I", 0xd9: ">B", 0xda: ">H", 0xdb: ">I", 0xdc: ">H", 0xdd: ">I", 0xde: ">H", 0xdf: ">I"}
    if t in lengths:
        w = struct.calcsize(lengths[t])
        n = struct.unpack(lengths[t], buf[pos:pos + w])[0]
        pos += w
        if t in (0xc4, 0xc5, 0xc6):
            return raw(n, pos, False)
        if t in (0xd9, 0xda, 0xdb):
            return raw(n, pos, True)
        return items(n, pos, t in (0xde, 0xdf))
    raise ValueError("msgpack type 0x%02x" % t)


def _elf_notes(elf):
    """(type, name, desc) of every note of a 64-bit little-endian ELF image"""
    assert elf[:6] == b"\x7fELF\x02\x01", "a 64-bit little-endian ELF"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3a)
    for i in range(shnum):
        _, sh_type, _, _, off, size = struct.unpack_from("<IIQQQQ", elf, shoff + i * shentsize)
        if sh_type != 7:   # SHT_NOTE
            continue
        pos, end = off, off + size
        while pos + 12 <= end:
            namesz, descsz, ntype = struct.unpack_from("<III", elf, pos)
            pos += 12
            name = elf[pos:pos + namesz].rstrip(b"\0")
            pos += (namesz + 3) & ~3
            yield ntype, name, elf[pos:pos + descsz]
            pos += (descsz + 3) & ~3


def kernel_metadata(library=None, arch="gfx950"):
    """{kernel symbol: its metadata map} for the arch's code objects bundled in the library"""
    blob = open(library or helpers.PRODUCT_LIB, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    kernels = {}
    start = blob.find(magic)
    while start >= 0:
        n, = struct.unpack_from("<Q", blob, start + len(magic))
        pos = start + len(magic) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
            triple = blob[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if arch in triple and size > 0:
                for ntype, name, desc in _elf_notes(blob[start + off:start + off + size]):
                    if ntype == 32 and name == b"AMDGPU":   # NT_AMDGPU_METADATA
                        for k in _msgpack(desc)[0]["amdhsa.kernels"]:
                            kernels[k[".name"]] = k
        start = blob.find(magic, start + len(magic))
    assert kernels, "no %s kernels in the library" % arch
    return kernels


def _one(kernels, stem):
    """the metadata of the kernels whose (mangled) name holds `stem`"""
    found = {n: k for n, k in kernels.items() if stem in n}
    assert found, stem
    return found


def _alloc(k):
    return -(-k[".vgpr_count"] // VGPR_GRANULE) * VGPR_GRANULE


def test_far_pair_kernel_fits_beside_two_strip_waves():
    kernels = kernel_metadata()
    strips, far = _one(kernels, "k_schur_window"), _one(kernels, "k_schur_blocks")
    for sn, s in strips.items():
        for fn, f in far.items():
            print(sn, s[".vgpr_count"], s[".group_segment_fixed_size"], fn, f[".vgpr_count"], f[".group_segment_fixed_size"], f[".private_segment_fixed_size"])
            assert 2 * _alloc(s) + _alloc(f) <= SIMD_VGPRS, (sn, s[".vgpr_count"], fn, f[".vgpr_count"])
            assert 2 * s[".group_segment_fixed_size"] + f[".group_segment_fixed_size"] <= CU_LDS_BYTES, (sn, s[".group_segment_fixed_size"], fn, f[".group_segment_fixed_size"])


def test_dense_bounding_box_kernel_has_no_private_segment():
    dense = _one(kernel_metadata(), "k_bbox_lin_dense")
    assert len(dense) == 2, sorted(dense)   # the 7- and the 9-parameter ellipsoid block
    for name, k in dense.items():
        print(name, k[".vgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"])
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".max_flat_workgroup_size"] == 256, (name, k[".max_flat_workgroup_size"])
