"""CPU: the C-ABI library loads and exports every function declared in include/ani_hip.h (no compute calls)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_symbol_is_exported():
    from lammps_ani_amd import ani_hip
    ani_hip.build()
    hdr = open(os.path.join(ROOT, "include", "ani_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ani_[a-z_0-9]+)\s*\(", hdr)))
    assert len(declared) >= 15
    lib = C.CDLL(ani_hip.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/ani_hip.h but not exported"
    assert set(ani_hip.EXPORTS) == set(declared)


def test_every_header_under_include_is_exported():
    """include/ani_md.h (the timestep loop's own kernels: not the drop-in boundary, but a C ABI of the same library)."""
    from lammps_ani_amd import ani_hip
    ani_hip.build()
    lib = C.CDLL(ani_hip.LIB_PATH)
    inc = os.path.join(ROOT, "include")
    seen = 0
    for name in sorted(os.listdir(inc)):
        if not name.endswith(".h"):
            continue
        hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, name)).read(), flags=re.S)
        for sym in sorted(set(re.findall(r"\b(ani_[a-z_0-9]+)\s*\(", hdr))):
            assert hasattr(lib, sym), f"{sym} declared in include/{name} but not exported"
            seen += 1
    assert seen >= 28


def test_makefile_objects_are_the_sources_of_csrc():
    """The library is linked from OBJS of csrc/Makefile: one object per *.hip and *.cpp of csrc, no other.  A unit left out of the
    list would show only as an unresolved symbol when the library is loaded.  The LAMMPS adapter (pair_ani.cpp, ani_plugin.cpp) is
    not part of the library: it is built against LAMMPS' headers into the plugin."""
    csrc = os.path.join(ROOT, "lammps-ani_amd", "csrc")
    adapter = {"pair_ani.cpp", "ani_plugin.cpp"}
    sources = sorted(n for n in os.listdir(csrc) if n.endswith((".hip", ".cpp")) and n not in adapter)
    assert len(sources) >= 20 and adapter <= set(os.listdir(csrc))
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    lists = re.findall(r"^OBJS\s*\+?=(.*)$", text, flags=re.M)
    assert lists
    objs = " ".join(lists).split()
    assert len(objs) == len(set(objs)), sorted(o for o in set(objs) if objs.count(o) > 1)
    assert sorted(objs) == sorted(os.path.splitext(n)[0] + ".o" for n in sources)
    assert len({os.path.splitext(n)[0] for n in sources}) == len(sources)   # no x.hip beside x.cpp: they would share an object


def test_create_fails_loudly_without_gpu_or_for_cpu_device(tmp_path):
    """No GPU in the build container: ani_create must return an error, never fall back."""
    import torch
    from lammps_ani_amd import ani_hip, model_file as mf
    p = str(tmp_path / "t.anim")
    mf.write_model(p, mf.synthetic_model("tiny", 1, 1))
    lib = ani_hip.lib()
    h = C.c_void_p()
    rc = lib.ani_create(p.encode(), -1, -1, 1, 1, 1, C.byref(h))
    assert rc != 0 and not h.value and b"cpu" in lib.ani_last_error(None)
    if not torch.cuda.is_available():
        rc = lib.ani_create(p.encode(), 0, -1, 1, 1, 1, C.byref(h))
        assert rc != 0 and not h.value and b"HIP device" in lib.ani_last_error(None)


def test_record_layouts_of_ani_md_h_and_ani_hip_py_agree():
    """The device records of include/ani_md.h are laid out once per language: the header's ANI_MD_*_ enums, and the *_LAYOUT tables of
    ani_hip.py that every Python reader goes through.  Same fields (an enum member without its prefix is a table's key, whatever
    the case), same first word, a field of several words ends where the next begins, and the counts agree."""
    from lammps_ani_amd import ani_hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ani_md.h")).read(), flags=re.S)
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(ANI_MD_\w+)\s+(\d+)\s*$", hdr, flags=re.M)}
    members = {}
    for body in re.findall(r"\benum\s*\{(.*?)\}", hdr, flags=re.S):
        value = -1
        for item in filter(None, (s.strip() for s in body.split(","))):
            name, _, given = (s.strip() for s in item.partition("="))
            value = int(given) if given else value + 1
            assert name not in members and name not in defines, name
            members[name] = value
    records = {"ANI_MD_FIRE_": (ani_hip.FIRE_LAYOUT, "ANI_MD_FIRE_NSTATE"), "ANI_MD_NH_": (ani_hip.NH_LAYOUT, "ANI_MD_NH_NSTATE"),
               "ANI_MD_THERMO_": (ani_hip.THERMO_LAYOUT, "ANI_MD_THERMO_N"), "ANI_MD_NPT_": (ani_hip.NPT_LAYOUT, "ANI_MD_NPT_NSTATE"),
               "ANI_MD_RESTRAINT_REC_": (ani_hip.RESTRAINT_LAYOUT, "ANI_MD_RESTRAINT_NREC")}
    assert all(any(name.startswith(p) for p in records) for name in members), sorted(members)
    for prefix, (table, count) in records.items():
        in_header = sorted((v, k[len(prefix):]) for k, v in members.items() if k.startswith(prefix))
        starts = {k.upper(): (at.start if isinstance(at, slice) else at) for k, at in table.items()}
        assert len(starts) == len(table) and starts == {k: v for v, k in in_header}, prefix
        ends = [v for v, _ in in_header[1:]] + [defines[count]]
        for (first, name), end in zip(in_header, ends):
            at = {k.upper(): at for k, at in table.items()}[name]
            assert first < end <= defines[count], (prefix, name)
            if isinstance(at, slice):
                assert (at.stop, at.step) == (end, None), (prefix, name)
    for py, c in (("FIRE_NSTATE", "ANI_MD_FIRE_NSTATE"), ("SHAKE_NSTATS", "ANI_MD_SHAKE_NSTATS"), ("NH_NSTATE", "ANI_MD_NH_NSTATE"),
                  ("NH_MAXCHAIN", "ANI_MD_NH_MAXCHAIN"), ("THERMO_N", "ANI_MD_THERMO_N"), ("NPT_NSTATE", "ANI_MD_NPT_NSTATE"),
                  ("RESTRAINT_NREC", "ANI_MD_RESTRAINT_NREC")):
        assert getattr(ani_hip, py) == defines[c], (py, c)
    assert len(ani_hip.SHAKE_STATS_KEYS) == defines["ANI_MD_SHAKE_NSTATS"]
    assert {k: v[0] for k, v in ani_hip.RESTRAINT_KINDS.items()} == {
        k: defines["ANI_MD_RESTRAINT_" + k.upper()] for k in ("distance", "angle", "torsion")}
    # the tuples that zip a whole record are in the record's order
    assert [ani_hip.FIRE_LAYOUT[k] for k in ani_hip.FIRE_STATE_KEYS] == list(range(defines["ANI_MD_FIRE_NSTATE"]))
    assert [ani_hip.THERMO_LAYOUT[k] for k in ani_hip.THERMO_KEYS] == list(range(len(ani_hip.THERMO_KEYS)))
