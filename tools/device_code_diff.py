#!/usr/bin/env python3
"""Is the device code of two builds of libqd_hip.so the same, kernel by kernel?

    python tools/device_code_diff.py OTHER_libqd_hip.so [THIS_libqd_hip.so]

For a change that touches host code only (a launcher, a header split) the answer must be yes: that is its whole speed argument.
The function symbols of all gfx950 code objects a library embeds (tools/kernel_meta.code_objects: one per translation unit)
are pooled by name, and for every name the machine-code bytes are compared, and so are the kernel descriptors (the 64-byte
`.kd` objects) and the metadata of tools/kernel_meta.kernels (VGPRs, SGPRs, LDS, scratch, spills).  Symbols may move, inside
a code object or from one translation unit to another; they may not change.  Exit status 1 on any difference."""
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kernel_meta  # noqa: E402


def symbols(img):
    """{name: bytes} of every FUNC / OBJECT symbol with a size in an ELF64 little-endian image (symtab, else dynsym)."""
    shoff, = struct.unpack_from('<Q', img, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', img, 0x3A)
    secs = [struct.unpack_from('<IIQQQQIIQQ', img, shoff + i * shentsize) for i in range(shnum)]
    tabs = [s for s in secs if s[1] == 2] or [s for s in secs if s[1] == 11]          # SHT_SYMTAB, SHT_DYNSYM
    out = {}
    for tab in tabs:
        strtab = secs[tab[6]]
        for off in range(tab[4], tab[4] + tab[5], 24):
            name_off, info, _other, shndx, value, size = struct.unpack_from('<IBBHQQ', img, off)
            if size == 0 or (info & 15) not in (1, 2) or shndx == 0 or shndx >= shnum:
                continue
            end = img.index(b'\0', strtab[4] + name_off)
            name = img[strtab[4] + name_off:end].decode()
            sec = secs[shndx]
            if sec[1] == 8:                                                           # SHT_NOBITS: nothing to compare but the size
                out[name] = b'<%d zero bytes>' % size
                continue
            start = sec[4] + (value - sec[3])
            out[name] = img[start:start + size]
    return out


def same_but_moved(name, x, y):
    """Equal up to the two places where a symbol's POSITION is encoded: the code entry offset of a kernel descriptor (bytes
    16 .. 23 of a `.kd`), and the 32-bit literals of the s_add_u32 / s_addc_u32 pair behind an s_getpc_b64 -- the
    PC-relative address of a device variable (k_single_fused: its barrier slots)."""
    if len(x) != len(y):
        return False
    if name.endswith('.kd'):
        return len(x) == 64 and x[:16] == y[:16] and x[24:] == y[24:]
    if len(x) % 4:
        return False
    wx, wy = struct.unpack('<%dI' % (len(x) // 4), x), struct.unpack('<%dI' % (len(y) // 4), y)
    for i in (i for i in range(len(wx)) if wx[i] != wy[i]):
        literal_of_add = i >= 1 and wx[i - 1] == wy[i - 1] and (wx[i - 1] & 0xFD80FF00) == 0x8000FF00     # s_add_u32 / s_addc_u32 sN, sM, literal
        after_getpc = any((w & 0xFF80FFFF) == 0xBE801C00 for w in wx[max(0, i - 5):i])                  # s_getpc_b64
        if not (literal_of_add and after_getpc):
            return False
    return True


def main():
    other = sys.argv[1]
    this = sys.argv[2] if len(sys.argv) > 2 else kernel_meta.os.path.join(HERE, '..', 'quantized_distillation_amd', 'libqd_hip.so')
    a, b = kernel_meta.code_objects(other), kernel_meta.code_objects(this)
    bad = []

    def pooled(objs):
        """{name: bytes} over all code objects of a library: a symbol may move between translation units.  (A kernel of a
        shared header is emitted by every translation unit that includes it: the same bytes each time.)"""
        pool = {}
        for i, img in enumerate(objs):
            for name, code in symbols(img).items():
                if name.startswith('__hip_cuid_'):                 # the translation unit's id, a hash of its source text
                    continue
                if name in pool and pool[name] != code and not same_but_moved(name, pool[name], code):
                    bad.append('%s is defined twice with different bytes (again in code object %d)' % (name, i))
                pool[name] = code
        return pool

    sx, sy = pooled(a), pooled(b)
    nsym = nbytes = nmoved = 0
    for name in sorted(set(sx) | set(sy)):
        if name not in sx or name not in sy:
            bad.append('%s only in %s' % (name, 'the other library' if name in sx else 'this library'))
        elif sx[name] != sy[name] and not same_but_moved(name, sx[name], sy[name]):
            bad.append('%s differs (%d / %d bytes)' % (name, len(sx[name]), len(sy[name])))
        else:
            nsym += 1
            nbytes += len(sx[name])
            nmoved += sx[name] != sy[name]
    ma, mb = ({k['name']: k for k in kernel_meta.kernels(lib)} for lib in (other, this))
    if ma != mb:
        bad.append('kernel metadata differs: %s' % [(ma.get(n), mb.get(n)) for n in sorted(set(ma) | set(mb)) if ma.get(n) != mb.get(n)][:5])
    print('%d / %d code objects, %d symbols (%d bytes of code, descriptors and device data) identical -- %d of them up to an encoded '
          'position (same_but_moved) -- metadata of %d kernels %s' % (len(a), len(b), nsym, nbytes, nmoved, len(mb), 'identical' if ma == mb else 'DIFFERENT'))
    print('\n'.join(bad) if bad else 'device code is the same')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
