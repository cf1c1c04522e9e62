"""Register / scratch / LDS use of the gfx950 kernels in a HIP object or shared library, read
on the host (no GPU): the offload bundle in the .hip_fatbin section is split into its code
objects and llvm-readelf --notes prints each kernel's metadata. Used to check a kernel change
for VGPR growth and scratch spills before spending GPU time.
usage: python scripts/kernel_resources.py deepfmkit_amd/dfmi_capi.o [name-substring ...]
       python scripts/kernel_resources.py --hash deepfmkit_amd/dfmi_capi.o
--hash: the gate of a host-only change. One sorted line per function symbol of the code object
(name, size, SHA-256 of its bytes; __hip_cuid_* left out: it is derived from the source text),
then the sorted resource lines. Two builds with the same device code print the same table,
whatever the order their kernels were instantiated in (the whole object and the .kd
descriptors, which hold layout-relative offsets, differ then). A kernel that calls an out-of-line
device function (the LM kernels call dfmi_sincos_lib) holds the distance to it in the s_add_u32
literal after s_getpc_b64 (rel32@lo + 4), which moves with the layout too: a word equal to that
distance from its own address is hashed as zero."""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path):
    data = open(path, "rb").read()
    out = []
    pos = 0
    while True:
        i = data.find(MAGIC, pos)
        if i < 0:
            break
        n, = struct.unpack_from("<Q", data, i + 24)
        p = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                out.append(data[i + off:i + off + size])
        pos = i + 32
    return out


def functions(co):
    """(name, size, sha256 of the bytes) of every FUNC symbol in .symtab of an ELF64 code object."""
    shoff, = struct.unpack_from("<Q", co, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", co, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", co, shoff + i * shentsize) for i in range(shnum)]
    funcs, names = [], set()
    for sec in secs:
        if sec[1] != 2:  # SHT_SYMTAB
            continue
        stroff = secs[sec[6]][4]
        for o in range(sec[4], sec[4] + sec[5], 24):
            name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", co, o)
            text = co[stroff + name:co.index(b"\0", stroff + name)].decode()
            names.add(text)
            if info & 0xF == 2 and 0 < shndx < shnum and not text.startswith("__hip_cuid_"):  # STT_FUNC, defined
                funcs.append((text, size, value, secs[shndx][4] + value - secs[shndx][3]))
    callees = [value for text, _, value, _ in funcs if text + ".kd" not in names]  # no descriptor: not a kernel
    out = []
    for text, size, value, at in funcs:
        words = list(struct.unpack_from(f"<{size // 4}I", co, at))
        for i, w in enumerate(words):
            if any(w == (c + 4 - (value + 4 * i)) & 0xFFFFFFFF for c in callees):
                words[i] = 0
        body = struct.pack(f"<{len(words)}I", *words) + co[at + size // 4 * 4:at + size]
        out.append((text, size, hashlib.sha256(body).hexdigest()))
    return sorted(out)


def main():
    hashes = sys.argv[1] == "--hash"
    if hashes:
        del sys.argv[1]
    pats = sys.argv[2:]
    lines = []
    for k, co in enumerate(code_objects(sys.argv[1])):
        if hashes:
            for name, size, digest in functions(co):
                print(f"func {name} size {size} sha256 {digest}")
        with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
            f.write(co)
        notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True,
                               text=True).stdout
        os.unlink(f.name)
        cur = {}
        for line in notes.splitlines():
            m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)", line)
            if not m:
                continue
            key, val = m.group(1), m.group(2).strip()
            if key == "agpr_count":  # a kernel's block starts (keys in alphabetical order)
                cur = {"agpr": val}
            elif key in ("group_segment_fixed_size", "private_segment_fixed_size", "sgpr_count", "vgpr_count",
                         "vgpr_spill_count", "sgpr_spill_count"):
                cur[key] = val
            elif key == "name" and not val.endswith(".kd"):
                cur["name"] = val
            elif key == "wavefront_size" and "name" in cur:  # ... and ends
                val = cur["name"]
                if not pats or any(s in val for s in pats):
                    lines.append(f"{val if hashes else val[:100]:100s} vgpr {cur.get('vgpr_count')} "
                                 f"agpr {cur.get('agpr')} spill {cur.get('vgpr_spill_count')} "
                                 f"scratch {cur.get('private_segment_fixed_size')} "
                                 f"lds {cur.get('group_segment_fixed_size')}")
                cur = {}
    print("\n".join(sorted(lines) if hashes else lines))


if __name__ == "__main__":
    main()
