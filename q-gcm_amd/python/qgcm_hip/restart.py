"""Restart dumps in the reference's wire format (SUBROUTINE resave, src/q-gcm.F:3053-3088; read back at
src/q-gcm.F:612-640): Fortran sequential unformatted records with 4-byte length markers,

    tyrs | po, pom | [pa, pam] | sst, sstm | ast, astm | hmixa, hmixam

`[pa, pam]` is absent in an ocean_only build; the atmospheric mixed-layer arrays are (nxta, nyta) and are written
even then (MODULE intrfac declares them unconditionally).  An atmos_only build leaves `po, pom` out instead:

    tyrs | pa, pam | sst, sstm | ast, astm | hmixa, hmixam

where sst, sstm (nxto, nyto) are the prescribed SST it holds.  All fields are fp64, Fortran order.
This is the on-disk contract either side of the device path: a host reads a dump, pushes po/pom (+ sst/sstm) with
set_p / oml_set_state, and writes one from get_state / oml_get_state."""
import struct

import numpy as np


class TruncatedRestart(EOFError, ValueError):
    """The file ends before the records asked for do: the EOFError it always was, and a ValueError like every other
    mismatch between a file and the layout it is read as (an atmos_only dump read as a coupled one ends one record
    early)."""


def _rec(f):
    head = f.read(4)
    if len(head) != 4:
        raise TruncatedRestart("restart file ends inside a record marker")
    (n,) = struct.unpack("<i", head)
    data = f.read(n)
    (m,) = struct.unpack("<i", f.read(4))
    if len(data) != n or m != n:
        raise ValueError("corrupt Fortran record (markers %d / %d, %d bytes read)" % (n, m, len(data)))
    return np.frombuffer(data, dtype="<f8")


def _put(f, *arrays):
    body = b"".join(np.asfortranarray(a, dtype="<f8").tobytes(order="F") for a in arrays)
    f.write(struct.pack("<i", len(body)))
    f.write(body)
    f.write(struct.pack("<i", len(body)))


def _read_atmos_only(path, cfg):
    nT, nA, nP = cfg.nxto * cfg.nyto, cfg.nxta * cfg.nyta, (cfg.nxta + 1) * (cfg.nyta + 1)
    with open(path, "rb") as f:
        t, pa, s, a, h = (_rec(f) for _ in range(5))
        if f.read(1):
            raise ValueError("restart file %s has more than the five records of an atmos_only dump" % path)
    nla = pa.size // (2 * nP)
    if t.size != 1 or nla < 2 or pa.size != 2 * nP * nla or s.size != 2 * nT or a.size != 2 * nA or h.size != 2 * nA:
        raise ValueError("restart file %s is not an atmos_only dump of grid %s" % (path, cfg.name))
    sha, shT, shA = (cfg.nxta + 1, cfg.nyta + 1, nla), (cfg.nxto, cfg.nyto), (cfg.nxta, cfg.nyta)
    r = lambda v, sh: np.asfortranarray(v.reshape(sh, order="F"))
    return dict(tyrs=float(t[0]), pa=r(pa[:nP * nla], sha), pam=r(pa[nP * nla:], sha), sst=r(s[:nT], shT),
                sstm=r(s[nT:], shT), ast=r(a[:nA], shA), astm=r(a[nA:], shA), hmixa=r(h[:nA], shA), hmixam=r(h[nA:], shA))


def read_restart(path, cfg, coupled=False, *, atmos_only=False):
    """-> dict(tyrs, po, pom, sst, sstm, ast, astm, hmixa, hmixam) of an ocean_only dump for grid `cfg`;
    coupled=True: the dump of a coupled build, which also carries pa, pam (nxta+1, nyta+1, 3).
    atmos_only=True: the dump of an atmos_only build, dict(tyrs, pa, pam, sst, sstm, ast, astm, hmixa, hmixam) with
    pa, pam (nxta+1, nyta+1, nla), nla from the record's length; cfg gives nxta, nyta and the SST's nxto, nyto."""
    if atmos_only:
        if coupled:
            raise ValueError("read_restart: a dump is either coupled or atmos_only")
        return _read_atmos_only(path, cfg)
    np3, nT, nA = cfg.nxpo * cfg.nypo * cfg.nlo, cfg.nxto * cfg.nyto, cfg.nxta * cfg.nyta
    with open(path, "rb") as f:
        t = _rec(f)
        p = _rec(f)
        pa = _rec(f) if coupled else None
        s = _rec(f)
        a = _rec(f)
        h = _rec(f)
    if t.size != 1 or p.size != 2 * np3 or s.size != 2 * nT or a.size != 2 * nA or h.size != 2 * nA:
        raise ValueError("restart file %s does not match grid %s" % (path, cfg.name))
    sh3, shT, shA = (cfg.nxpo, cfg.nypo, cfg.nlo), (cfg.nxto, cfg.nyto), (cfg.nxta, cfg.nyta)
    r = lambda v, sh: np.asfortranarray(v.reshape(sh, order="F"))
    out = dict(tyrs=float(t[0]), po=r(p[:np3], sh3), pom=r(p[np3:], sh3), sst=r(s[:nT], shT), sstm=r(s[nT:], shT),
               ast=r(a[:nA], shA), astm=r(a[nA:], shA), hmixa=r(h[:nA], shA), hmixam=r(h[nA:], shA))
    if coupled:
        sha = (cfg.nxta + 1, cfg.nyta + 1, 3)
        na3 = sha[0] * sha[1] * sha[2]
        if pa.size != 2 * na3:
            raise ValueError("restart file %s: atmospheric record does not match grid %s" % (path, cfg.name))
        out.update(pa=r(pa[:na3], sha), pam=r(pa[na3:], sha))
    return out


def write_restart(path, cfg, tyrs, po=None, pom=None, sst=None, sstm=None, ast=None, astm=None, hmixa=None, hmixam=None,
                  pa=None, pam=None, *, atmos_only=False):
    """pa, pam given: the dump of a coupled build (record [pa, pam] after [po, pom]).  atmos_only=True: the dump of an
    atmos_only build, which has no [po, pom] record: pa, pam (nxta+1, nyta+1, nla) are required, po / pom refused."""
    zT, zA = np.zeros((cfg.nxto, cfg.nyto)), np.zeros((cfg.nxta, cfg.nyta))
    d = lambda x, z: z if x is None else x
    if atmos_only:
        if po is not None or pom is not None:
            raise ValueError("an atmos_only dump has no po / pom")
        sha = np.shape(pa)
        if len(sha) != 3 or sha[:2] != (cfg.nxta + 1, cfg.nyta + 1) or sha[2] < 2 or np.shape(pam) != sha:
            raise ValueError("pa / pam must be (%d, %d, nla)" % (cfg.nxta + 1, cfg.nyta + 1))
        for x, z in ((sst, zT), (sstm, zT), (ast, zA), (astm, zA), (hmixa, zA), (hmixam, zA)):
            if x is not None and np.shape(x) != z.shape:
                raise ValueError("a mixed-layer field has shape %s, need %s" % (np.shape(x), z.shape))
        with open(path, "wb") as f:
            _put(f, np.array([tyrs], dtype=np.float64))
            _put(f, pa, pam)
            _put(f, d(sst, zT), d(sstm, zT))
            _put(f, d(ast, zA), d(astm, zA))
            _put(f, d(hmixa, zA), d(hmixam, zA))
        return
    for x, sh in ((po, (cfg.nxpo, cfg.nypo, cfg.nlo)), (pom, (cfg.nxpo, cfg.nypo, cfg.nlo))):
        if np.shape(x) != sh:
            raise ValueError("po / pom must be %s" % (sh,))
    with open(path, "wb") as f:
        _put(f, np.array([tyrs], dtype=np.float64))
        _put(f, po, pom)
        if pa is not None:
            _put(f, pa, pam)
        _put(f, d(sst, zT), d(sstm, zT))
        _put(f, d(ast, zA), d(astm, zA))
        _put(f, d(hmixa, zA), d(hmixam, zA))
