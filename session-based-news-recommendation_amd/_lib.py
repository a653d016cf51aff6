"""Loader (and in-tree builder) of ``libtcar_hip.so`` — the C-ABI of include/tcar_hip.h.

The product path has NO CPU fallback: if the shared library is missing or a symbol is absent, importing the
engine raises.  `build()` cross-compiles the HIP sources for gfx950 with hipcc (works without a GPU).

Nothing of the ABI is restated here: the constants, the ctypes mirrors of the structs (Dims, Batch, Ctx, ...) and the prototype of
every entry point are read from the header itself (`_bind`), in `load()` or on first use of one of those names.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
from typing import List

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
# (TCAR_LIB: load THIS binary instead — a diagnostic build of the same sources, e.g. tools/obs1_probe.py's -DTCAR_OBS1_DIAG library;
#  it must carry the same source digest and ABI, and it is never built or overwritten by build())
LIB_PATH = os.environ.get("TCAR_LIB") or os.path.join(PKG_DIR, "libtcar_hip.so")
SOURCES = ["gemm_f32.hip", "gemm_bf16.hip", "embed.hip", "pool.hip", "score.hip", "ce.hip", "optim.hip", "step.hip", "mha.hip",
           "sampler.hip", "norm.hip", "shard.hip", "segsum.hip", "query.hip", "select.hip", "cand.hip", "retrieve.hip",
           "sections.hip", "catalog.hip", "mmr.hip", "similar.hip", "dupes.hip", "warm.hip", "buildid.hip"]
BUILD_ID_TU = "buildid.hip"        # the one translation unit that carries the digest of all sources


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


# The C ABI, one row per layer: (prefix of the layer's names in this module, its header under include/).  Every header is compiled
# into the library AND read by _bind(), and each builds on the rows above it: the core; in-place updates of catalog rows in a live
# context (on the core alone, so it sits next to it) and their ownership-aware form for a rank that holds a shard of the candidate
# side; streamed score-and-select; its publish-time
# windows; its per-category caps; one list per category from one pass (bound before the ragged layer, so its ragged twin takes the
# ragged descriptor as a plain pointer); the state merge and the shard's fold of the catalog-sharded serving path; candidate-list scoring;
# warm start (tcar_warm.h: item rows of cold articles blended from their related items' rows and installed by the catalog update; bound
# before the layers whose descriptors it names — its struct holds them as plain pointers —, as the sections are before the ragged layer);
# the streamed top-C shortlist and the two-stage step; its diversified close (the MMR walk over content; bound before the ragged
# layer, like the sections); related items by content cosine (the cosine panels of tcar_similar.h under the folds of the serving layers);
# the all-pairs duplicate audit over the same cosine (tcar_dupes.h: its own kernels, on the tile of the panels);
# the shortlist merge, the owner-aware candidate gather and the shard's side of both on the catalog-sharded engine; ragged batches (sessions of mixed lengths) under every serving step.
ABI_LAYERS = [("", "tcar_hip.h"), ("CATALOG", "tcar_catalog.h"), ("CATALOG_SHARD", "tcar_catalog_shard.h"), ("SERVE", "tcar_serve.h"),
              ("WINDOW", "tcar_window.h"), ("QUOTA", "tcar_quota.h"), ("SECTIONS", "tcar_sections.h"),
              ("SERVE_SHARD", "tcar_serve_shard.h"), ("CAND", "tcar_cand.h"), ("WARM", "tcar_warm.h"), ("RETRIEVE", "tcar_retrieve.h"),
              ("MMR", "tcar_mmr.h"), ("SIMILAR", "tcar_similar.h"), ("DUPES", "tcar_dupes.h"), ("RETRIEVE_SHARD", "tcar_retrieve_shard.h"),
              ("RAGGED", "tcar_ragged.h")]


def _name(prefix: str, name: str) -> str:
    """the module name `name` of the layer `prefix`: HEADER / SERVE_HEADER, SYMBOLS / SERVE_SYMBOLS, ..."""
    return prefix + "_" + name if prefix else name


for _prefix, _file in ABI_LAYERS:          # HEADER, SERVE_HEADER, WINDOW_HEADER, QUOTA_HEADER, SERVE_SHARD_HEADER, CAND_HEADER, ...
    globals()[_name(_prefix, "HEADER")] = os.path.join(PKG_DIR, "..", "include", _file)
HEADERS = [os.path.join(CSRC, "tcar_common.h"), os.path.join(CSRC, "tcar_bf16_layout.h"), os.path.join(CSRC, "topk_rows.h"),
           os.path.join(CSRC, "ce_rows.h"), os.path.join(CSRC, "panel_fold.h"), os.path.join(CSRC, "sim_tile.h")] + \
    [globals()[_name(_prefix, "HEADER")] for _prefix, _ in ABI_LAYERS]
_ID_MARK = b"TCAR_BUILD_ID="


def _digest(paths) -> str:
    import hashlib
    h = hashlib.sha256()
    for p in paths:
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:32]


def source_build_id() -> str:
    """Digest of every source the library is compiled from (csrc/*.hip, the csrc headers, include/*.h) and of the
    code-generation flags every translation unit must be built with (SAFE_FLAGS): a binary built without them is stale."""
    import hashlib
    base = _digest([os.path.join(CSRC, s) for s in SOURCES] + HEADERS)
    return hashlib.sha256((base + "|" + " ".join(SAFE_FLAGS)).encode()).hexdigest()[:32]


def binary_build_id(path: str = LIB_PATH):
    """The digest baked into a built libtcar_hip.so (tcar_build_id()), read from the file without loading it."""
    try:
        with open(path, "rb") as f:
            blob = f.read()
    except OSError:
        return None
    i = blob.find(_ID_MARK)
    if i < 0:
        return None
    j = blob.find(b"\0", i)
    return blob[i + len(_ID_MARK):j].decode(errors="replace")


# Every translation unit is compiled WITHOUT the SLP vectorizer.  hipcc 7.2 at -O3 packs adjacent scalar f32 FMAs into v_pk_fma_f32 with
# operand selects, and on gfx950 `v_pk_fma_f32 ... op_sel:[0,1,0]` (the low result takes the HIGH dword of the second source: what
# the vectorizer emits for `acc = fma(row, s[r], acc)` with four consecutive s) loses its low-half product in lanes 48-63, now and
# then, while another wave of the same SIMD issues MFMAs — DESIGN.md §7 observation 1; repro tools/micro/pkfma_lds.hip and
# tools/obs1_probe.py, evidence profiles/r05_obs1_erratum.txt.  The step co-schedules such kernels with the scoring GEMMs on
# purpose.  Measured perf-neutral (profiles/r05_ab_experiments.txt); tests/test_host_logic.py scans the built binary for the form.
SAFE_FLAGS = ["-fno-slp-vectorize"]


def have_sources() -> bool:
    return all(os.path.exists(os.path.join(CSRC, s)) for s in SOURCES) and all(os.path.exists(h) for h in HEADERS)


def build(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 -O3 -shared -fPIC csrc/*.hip -> libtcar_hip.so (in-tree).  The digest of the sources
    is compiled in (tcar_build_id); a library whose digest differs from the sources next to it is rebuilt.  Objects are
    cached per source file (digest of the file + headers), so an edit recompiles one translation unit."""
    if not have_sources():
        raise FileNotFoundError("HIP sources missing under " + CSRC)
    want = source_build_id()
    if os.environ.get("TCAR_LIB"):
        # a diagnostic binary named by TCAR_LIB is only ever VERIFIED here: build() never links over it (its flags differ from
        # SAFE_FLAGS on purpose — tools/micro/build_obs1.sh), a stale one is an error, not something to overwrite
        if not os.path.exists(LIB_PATH) or binary_build_id() != want:
            raise RuntimeError("TCAR_LIB=%s does not carry the digest of the sources next to it (%s): rebuild it with the script "
                               "that made it, or unset TCAR_LIB" % (LIB_PATH, want))
        return LIB_PATH
    if not force and os.path.exists(LIB_PATH) and binary_build_id() == want:
        return LIB_PATH
    objs = []
    procs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        o = os.path.join(CSRC, s.replace(".hip", ".o"))
        objs.append(o)
        extra = os.environ.get("TCAR_HIPCC_FLAGS", "").split()      # e.g. -DTCAR_GEMM_DIAG (diagnostic kernel forms, tools/gemm_variants.sh)
        dig = _digest([src] + HEADERS) + (":" + want if s == BUILD_ID_TU else "") + ":" + " ".join(SAFE_FLAGS + extra)
        stamp = o + ".digest"
        if not force and os.path.exists(o) and os.path.exists(stamp) and open(stamp).read() == dig:
            continue
        cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17"] + SAFE_FLAGS + extra + ["-c", src, "-o", o]
        if s == BUILD_ID_TU:
            cmd.insert(1, '-DTCAR_BUILD_ID="%s"' % want)
        procs.append((cmd, stamp, dig, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for cmd, stamp, dig, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), out.decode(errors="replace")))
        with open(stamp, "w") as f:
            f.write(dig)
        if verbose and out:
            print(out.decode(errors="replace"))
    link = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
    r = subprocess.run(link, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("link failed: %s\n%s" % (" ".join(link), r.stdout.decode(errors="replace")))
    return LIB_PATH


# ------------------------------------------------------------------ bindings, generated from include/tcar_hip.h
class TcarError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float}
# tcar_x_t -> public class name where CamelCase of x is not it
_CLASS_NAMES = {"tcar_negsrc_t": "NegSrc"}
# structs whose pointers stay c_void_p in the prototypes: callers pass arrays cast to c_void_p, integer addresses and None
_OPAQUE = ("tcar_tuning_t", "tcar_colsum_t", "tcar_fold_t")
_TYPE = re.compile(r"\s*(?:const\s+)?(\w+)")         # the type word a declaration starts with, `const` aside


def _read_header(path: str, const: dict, structs: dict):
    """One header of the C ABI -> its constants and structs (added to `const` / `structs`, which may hold those of a header it
    includes) and {function: (restype, argtypes)}.  Returns (public struct classes by name, prototypes)."""
    try:
        with open(path) as f:
            text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    except OSError as e:
        raise TcarError("the bindings are generated from %s, which cannot be read (%s)" % (os.path.normpath(path), e))
    const.update({k: int(v) for k, v in re.findall(r"^#define (TCAR_\w+) (\d+)\s*$", text, flags=re.M)})
    v = -1
    enum = re.search(r"enum \{([^}]*)\}", text)
    for item in enum.group(1).split(",") if enum else ():
        name, _, val = item.partition("=")
        const[name.strip()] = v = int(val) if val.strip() else v + 1

    classes = {}
    for body, cname in re.findall(r"typedef struct \{([^{}]*)\}\s*(tcar_\w+_t)\s*;", text):
        fields = []
        for decl in filter(str.strip, body.split(";")):
            m = _TYPE.match(decl)
            base = m.group(1)
            for d in decl[m.end():].split(","):                # `* E` | ` lda[3]`, ` ldb[3]` | ` *x_icp`, ` *x_pt` | `* const* ev_start`
                name, dim = re.search(r"(\w+)\s*(?:\[(\w+)\])?\s*$", d).groups()
                t = C.c_void_p if "*" in d else _SCALARS.get(base) or structs[base]
                fields.append((name, t * (int(dim) if dim.isdigit() else const[dim]) if dim else t))
        pub = _CLASS_NAMES.get(cname) or "".join(w.capitalize() for w in cname[5:-2].split("_"))
        structs[cname] = classes[pub] = type(pub, (C.Structure,), {"_fields_": fields, "__doc__": "mirror of " + cname, "__module__": __name__})

    def ctype(decl: str, ret: bool = False):
        base = _TYPE.match(decl).group(1)
        if "*" not in decl:
            return _SCALARS[base]
        if "[" in decl:                                       # T* const name[5]
            return C.POINTER(C.c_void_p * int(re.search(r"\[(\d+)\]", decl).group(1)))
        if base == "char":
            return C.c_char_p
        return C.POINTER(structs[base]) if base in structs and base not in _OPAQUE and not ret else C.c_void_p

    protos = {}
    for ret, name, params in re.findall(r"^((?:const )?\w+\*?) (tcar_\w+)\(([^)]*)\)\s*;", text, flags=re.M):
        params = [] if params.strip() == "void" else params.split(",")
        protos[name] = (ctype(ret, True), [ctype(p) for p in params])
    return classes, protos


def _bind() -> None:
    """Read the C ABI from the headers of ABI_LAYERS, in order: the constants, one ctypes.Structure per `typedef struct` (header order,
    so nested structs resolve) and (restype, argtypes) of every declared function.  Each layer is read on top of the constants and
    structs of the layers above it and publishes, as attributes of this module, <PREFIX>_SYMBOLS, <PREFIX>_ABI_VERSION and its
    struct mirrors (the core layer, without a prefix: SYMBOLS, ABI_VERSION, Dims, Ctx, ...); the prototypes of all layers go into
    _PROTOTYPES.  Once."""
    g = globals()
    if "SYMBOLS" in g:
        return
    const, structs, out = {}, {}, {"_PROTOTYPES": {}}
    for prefix, _ in ABI_LAYERS:
        classes, protos = _read_header(g[_name(prefix, "HEADER")], const, structs)
        out.update(classes)
        out[_name(prefix, "SYMBOLS")] = list(protos)
        out[_name(prefix, "ABI_VERSION")] = const["TCAR_" + _name(prefix, "ABI_VERSION")]
        out["_PROTOTYPES"].update(protos)
    g.update(out, NSLOT=const["TCAR_NSLOT"], NVAR=const["TCAR_NVAR"], TUNING_FIELDS=[f[0] for f in out["Tuning"]._fields_])


def __getattr__(name: str):
    """ABI_VERSION, SYMBOLS, Dims, Ctx, ... for an importer that asks before load(): the header is read on first use"""
    if name.startswith("__"):
        raise AttributeError(name)
    _bind()
    try:
        return globals()[name]
    except KeyError:
        raise AttributeError("module %r has no attribute %r" % (__name__, name)) from None


def tuning(**overrides) -> "Tuning":
    """The process-wide switch values (shipped defaults + TCAR_* environment) with `overrides` applied, e.g.
    tuning(TCAR_BF16_TILE=384) or tuning(bf16_tile=384).  The library itself keeps no mutable switch."""
    lib = load()
    t = Tuning()
    check(lib.tcar_tuning_defaults(C.byref(t)), "tcar_tuning_defaults")
    for k, v in overrides.items():
        if k.startswith("TCAR_"):
            if lib.tcar_tuning_set(C.byref(t), k.encode(), int(v)) == -2 ** 31:
                raise KeyError(k)
        else:
            if k not in TUNING_FIELDS:
                raise KeyError(k)
            setattr(t, k, int(v))
    return t


_LIB = None


def load() -> C.CDLL:
    """dlopen the in-tree library, check that every declared symbol is exported and give each its prototype."""
    global _LIB
    if _LIB is not None:
        return _LIB
    _bind()
    # The library must bind to the SAME HIP runtime instance that owns the caller's device pointers and streams.
    # PyTorch-ROCm bundles its own libamdhip64; importing torch first makes the dynamic loader resolve our
    # DT_NEEDED libamdhip64.so.N to that already-loaded copy (two runtimes in one process => hipErrorNoDevice).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise TcarError("libtcar_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'`; "
                        "there is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    g = globals()
    missing = [s for prefix, _ in ABI_LAYERS for s in g[_name(prefix, "SYMBOLS")] if not hasattr(lib, s)]
    if missing:
        raise TcarError("libtcar_hip.so lacks symbols: %s" % missing)
    for s, (restype, argtypes) in _PROTOTYPES.items():
        f = getattr(lib, s)
        f.restype, f.argtypes = restype, argtypes
    for prefix, _ in ABI_LAYERS:           # tcar_abi_version, tcar_serve_abi_version, ...: "serve ABI", ..., "serve-shard ABI"
        got, want = getattr(lib, "tcar_" + _name(prefix.lower(), "abi_version"))(), g[_name(prefix, "ABI_VERSION")]
        if got != want:
            raise TcarError("libtcar_hip.so has %sABI %d, these bindings expect %d: rebuild%s"
                            % (prefix and prefix.lower().replace("_", "-") + " ", got, want,
                               "" if prefix else " (python -c 'import __graft_entry__ as g; g.build()')"))
    # a binary built from other sources than the ones next to it is stale (the build is digest-gated, not mtime-gated)
    if have_sources():
        got, want = lib.tcar_build_id().decode(), source_build_id()
        if got != want:
            raise TcarError("libtcar_hip.so was built from other sources (build id %s, sources %s): rebuild with "
                            "python -c 'import __graft_entry__ as g; g.build()'" % (got, want))
    _LIB = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise TcarError("%s failed with code %d (%s)" % (what, rc, {-1: "bad argument", -2: "launch error"}.get(rc, "?")))
