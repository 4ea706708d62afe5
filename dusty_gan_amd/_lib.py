"""ctypes binding of libdustygan_hip.so (the C ABI declared in include/dusty_gan_hip.h).

The header is the one statement of that boundary: at import `read_header` takes every prototype, struct and integer code
from it (PROTOTYPES, DgConv ... DgOptSeg, DG_*), so a new entry point is declared there and nowhere else.  The module
imports without torch and without the built library.

There is deliberately NO fallback: if the HIP library is missing, importing the product path raises.
PyTorch is used only as the owner of device memory and of the HIP stream.
"""
import ctypes as C
import keyword
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libdustygan_hip.so")
if os.environ.get("DUSTY_GAN_LIB_DIAG"):  # kernel-development aid: `make -C csrc diag` (ablation switches, stamps);
    _d = os.environ["DUSTY_GAN_LIB_DIAG"]  # "1" or the suffix of a renamed copy (libdustygan_hip_diag<suffix>.so)
    LIB_PATH = os.path.join(CSRC, "libdustygan_hip_diag%s.so" % ("" if _d == "1" else _d))
HEADER = os.path.join(os.path.dirname(_HERE), "include", "dusty_gan_hip.h")


class DgError(RuntimeError):
    pass


# C type of a by-value argument or struct field -> ctypes type; every pointer is a c_void_p, but for an ARGUMENT that points
# to a struct of the header: POINTER(that struct)
_SCALARS = {"int": C.c_int, "long": C.c_long, "long long": C.c_longlong, "unsigned": C.c_uint,
            "unsigned long long": C.c_ulonglong, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float,
            "double": C.c_double, "unsigned char": C.c_ubyte, "unsigned short": C.c_ushort}
_C_WORDS = frozenset("const void char short int long unsigned signed float double struct enum".split())


def read_header(text):
    """(constants, structs, prototypes) of a C header written like include/dusty_gan_hip.h:
    constants   {name: int} of every `#define DG_<NAME> <integer expression>` (earlier constants in scope) and of the entries
                of `enum { ... }` blocks
    structs     {name: ctypes.Structure subclass} of every `typedef struct X { ... } X;`, fields in the header's order, a
                field named like a Python keyword with a trailing underscore (`in` -> `in_`)
    prototypes  {name: (restype, [argtypes])} of every `int dg_x(...);` / `const char* dg_x(void);`
    Strict: DgError, naming the declaration, for anything it does not understand - it never guesses a type."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text.replace("\\\n", " "), flags=re.S)
    constants, structs, prototypes = {}, {}, {}

    def integer(expr, what):
        """a C integer expression of literals, operators and earlier constants (nothing else passes the character check)"""
        src = re.sub(r"\b(0[xX][0-9a-fA-F]+|\d+)[uUlL]*\b", r"\1", expr).replace("/", "//")
        try:
            if not src.strip() or re.search(r"[^\w\s()+\-*/%<>|&^~]", src):
                raise ValueError("not an integer expression")
            value = eval(src, {"__builtins__": {}}, dict(constants))
            if type(value) is not int:
                raise ValueError("not an integer")
        except Exception as e:
            raise DgError(f"{what}: cannot evaluate `{expr.strip()}` ({e})") from None
        return value

    def declared(decl, what, arg):
        """[(name, ctypes type)] of `type declarator {, declarator}`: one argument (arg) or one field declaration"""
        dims = r"((?:\[\s*\w+\s*\]\s*)*)"
        shown = " ".join(decl.split())
        first, *more = [d.strip() for d in decl.split(",")]
        m = re.fullmatch(r"(.*?)(\w+)\s*" + dims, first, flags=re.S)
        rest = [re.fullmatch(r"(\**)\s*(\w+)\s*" + dims, d) for d in more]
        if not m or None in rest:
            raise DgError(f"{what}: cannot read `{shown}`")
        base = " ".join(w for w in m.group(1).replace("*", " ").split() if w != "const")
        items = [(m.group(1).count("*"), m.group(2), m.group(3))] + [(len(r.group(1)), r.group(2), r.group(3)) for r in rest]
        if not base or any(name in _C_WORDS for _, name, _ in items) or (arg and items[0][2]):
            raise DgError(f"{what}: cannot read `{shown}`")
        if base not in _SCALARS and base not in structs and base != "void":
            raise DgError(f"{what}: the type `{base}` of `{shown}` is not one the binding knows")
        out = []
        for stars, name, dim in items:
            if stars:
                t = C.POINTER(structs[base]) if arg and stars == 1 and base in structs else C.c_void_p
            elif base in _SCALARS:
                t = _SCALARS[base]
            else:
                raise DgError(f"{what}: `{base}` by value in `{shown}` is not a type the binding knows")
            for n in reversed(re.findall(r"\w+", dim)):
                t = t * integer(n, what)
            out.append((name + "_" if keyword.iskeyword(name) else name, t))
        return out

    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(DG_\w+)(.*)$|\benum\s*\w*\s*\{([^{}]*)\}", text, flags=re.M):
        entries, nxt = [], 0
        if m.group(1):
            if m.group(2).startswith("("):
                raise DgError(f"#define {m.group(1)}: a macro with arguments is not a constant")
            entries.append((m.group(1), integer(m.group(2), "#define " + m.group(1))))
        for ent in (m.group(3) or "").split(","):
            name, eq, expr = (s.strip() for s in ent.partition("="))
            if name:
                nxt = integer(expr, "enum entry " + name) if eq else nxt
                entries.append((name, nxt))
                nxt += 1
        for name, value in entries:
            if not re.fullmatch(r"DG_\w+", name) or constants.setdefault(name, value) != value:
                raise DgError(f"constant {name}: not a DG_ name, or defined twice with different values")

    for m in re.finditer(r"\btypedef\s+struct\s*(\w*)\s*\{(.*?)\}\s*(\w*)\s*;", text, flags=re.S):
        name, body, alias = m.groups()
        where = f"struct {name or alias}"
        fields = [f for decl in body.split(";") if decl.strip() for f in declared(decl, where, False)]
        if not name or alias != name or not fields or name in structs:
            raise DgError(f"{where}: cannot split `typedef struct {name} {{...}} {alias};` into fields")
        structs[name] = type(name, (C.Structure,), {"_fields_": fields})

    def function(m):
        ret, name, params = " ".join(m.group(1).split()), m.group(2), m.group(3).strip()
        restype = C.c_char_p if ret.replace(" ", "") == "constchar*" else _SCALARS.get(ret)
        if restype is None:
            raise DgError(f"{name}: the return type `{ret}` is not one the binding knows")
        args = [] if params in ("", "void") else [declared(p, name, True)[0][1] for p in params.split(",")]
        if prototypes.setdefault(name, (restype, args)) != (restype, args):
            raise DgError(f"{name}: declared twice with different prototypes")
        return " "

    rest = re.sub(r"\b([\w \t]+?\**)\s*\b(dg_\w+)\s*\(([^()]*)\)\s*;", function, text)
    m = re.search(r"\bdg_\w+\s*\([^;]*", rest)
    if m:
        raise DgError(f"`{' '.join(m.group(0).split())[:120]}`: a dg_ declaration the binding cannot read")
    return constants, structs, prototypes


try:
    with open(HEADER) as _f:
        _CONSTANTS, _STRUCTS, _SIGNATURES = read_header(_f.read())
except OSError as _e:
    raise DgError(f"{HEADER}: the header that declares the C ABI cannot be read ({_e})") from None
globals().update(_CONSTANTS)   # every DG_* of the header
globals().update(_STRUCTS)     # DgConv ... DgOptSeg
PROTOTYPES = {_name: _argtypes for _name, (_, _argtypes) in _SIGNATURES.items()}   # name -> argtypes

MODE_S2, MODE_UP, MODE_GEMM = DG_MODE_S2, DG_MODE_UP, DG_MODE_GEMM
EPI_LINEAR, EPI_LRELU, EPI_MASK = DG_EPI_LINEAR, DG_EPI_LRELU, DG_EPI_MASK
UP_FRAG_BYTES = DG_UP_FRAG_BYTES
DBIAS_WS_FLOATS = DG_DBIAS_SLOTS * DG_DBIAS_SLOT_FLOATS
XSUM_PARTS = DG_XSUM_PARTS       # partial sums per sample where a producer leaves them un-summed
EXPORT_CHUNK = DG_EXPORT_CHUNK   # the pixels per workgroup of dg_export_points (sizes its chunk_counts workspace)
OPT_MAX_SEG = DG_OPT_MAX_SEG
POLICY_BITS = {"brightness": 1, "saturation": 2, "contrast": 4, "translation": 8, "cutout": 16}   # a comment in the header

_ERR = {DG_EINVAL: "DG_EINVAL (bad argument)", DG_EUNSUPPORTED: "DG_EUNSUPPORTED (shape not supported by the requested kernel)",
        DG_EHIP: "DG_EHIP (HIP runtime error)"}

_lib = None


def build(verbose=False):
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1))]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise DgError("building libdustygan_hip.so failed:\n" + res.stdout[-4000:] + res.stderr[-4000:])
    if verbose:
        print(res.stdout)
    return LIB_PATH


def build_diag(bits=8):
    """The diagnostic twin of the library (libdustygan_hip_diag.so: the ping-pong conv with cycle stamps; `make diag`).  Never
    loaded by the product path, the tests or the timed region: scripts/conv_clock.py reads the clock the chip holds inside
    the conv kernel from it (bench.py `roofline.clock_ghz`).  Returns its path, or None when the build fails (a missing
    diagnostic library costs one key of the bench line, never the line)."""
    res = subprocess.run(["make", "-C", CSRC, "diag", f"DIAGBITS={int(bits)}"], capture_output=True, text=True)
    path = os.path.join(CSRC, "libdustygan_hip_diag.so")
    return path if res.returncode == 0 and os.path.exists(path) else None


def lib():
    """Load (once) and return the ctypes handle.  Raises DgError when the library is absent: no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DgError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C dusty_gan_amd/csrc`). "
            "There is no CPU or PyTorch fallback for the hot path.")
    h = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(h, name)  # AttributeError if the symbol is not exported
        fn.argtypes = argtypes
        fn.restype = restype
    _lib = h
    return h


def check(rc, what=""):
    if rc != DG_OK:
        raise DgError(f"{what or 'libdustygan_hip call'} failed: {_ERR.get(rc, rc)}")


def dtype_code(t):
    import torch
    if t == torch.float32:
        return DG_F32
    if t == torch.bfloat16:
        return DG_BF16
    raise DgError(f"unsupported dtype {t}")


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else t.data_ptr()


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


def zero_(t):
    """t.zero_() as a kernel of this library (fp32 tensors; see dg_zero in include/dusty_gan_hip.h)"""
    import torch
    assert t.dtype == torch.float32 and t.is_contiguous()
    check(lib().dg_zero(t.data_ptr(), t.numel(), stream_ptr()), "dg_zero")
    return t


def zero_multi(tensors):
    """zero-fill up to 4 contiguous fp32 tensors (numel % 4 == 0) in one launch"""
    import ctypes as C
    import torch
    ts = [t for t in tensors if t is not None and t.numel() > 0]
    for i in range(0, len(ts), 4):
        chunk = ts[i:i + 4]
        assert all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() % 4 == 0 for t in chunk)
        ptrs = (C.c_void_p * len(chunk))(*[t.data_ptr() for t in chunk])
        cnts = (C.c_long * len(chunk))(*[t.numel() for t in chunk])
        check(lib().dg_zero_multi(ptrs, cnts, len(chunk), stream_ptr()), "dg_zero_multi")


def step_prologue(tensors, draws, fetch=None):
    """zero-fill up to 4 contiguous fp32 tensors and run up to 6 DgDraw jobs in ONE launch (dg_step_prologue); fetch: a DgFetch -
    fetch_reals of the step's batch as more workgroups of the same launch (dg_step_prologue_fetch)"""
    import ctypes as C
    import torch
    ts = [t for t in tensors if t is not None and t.numel() > 0]
    assert len(ts) <= 4 and len(draws) <= 6
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() % 4 == 0 for t in ts)
    ptrs = (C.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])
    cnts = (C.c_long * max(len(ts), 1))(*[t.numel() for t in ts])
    arr = (DgDraw * max(len(draws), 1))(*draws)
    if fetch is not None:
        check(lib().dg_step_prologue_fetch(ptrs, cnts, len(ts), arr, len(draws), C.byref(fetch), stream_ptr()),
              "dg_step_prologue_fetch")
        return
    check(lib().dg_step_prologue(ptrs, cnts, len(ts), arr, len(draws), stream_ptr()), "dg_step_prologue")


class AccArena:
    """Small fp32 accumulators that must start at zero (per-sample sums, logits, the logged scalars), carved from ONE
    buffer per DEVICE that one kernel zero-fills at the start of a training step - instead of one ~5 us zero-fill node per
    accumulator (11 per step).  `take(n)` hands out a slice that has been zero since the last `begin()` and is handed
    out once; None when the arena is not in use or exhausted (the caller then uses the self-zeroing entry point).
    Round 6: one arena (+ fixed-point shadow) per device, allocated once and kept for the life of the process: a captured
    hipGraph holds raw pointers into it, and the library's per-device registration (dg_det_arena) points at it - a second
    trainer on another device gets that device's own arena instead of re-allocating (and silently un-registering) the first
    one's (round-5 review, item 7).  Trainers that share a device share its arena: their steps are ordered on the device, and
    every step opens its epoch with a zero-fill."""
    SIZE = 8192
    buf, pos, epoch = None, 0, 0               # the arena of the device `begin` was last called for; epoch counts begin() calls
    shadow = None                              # fixed-point shadow words of the slots (deterministic cross-block sums)
    _by_dev = {}                               # device index -> (buf, shadow)

    @staticmethod
    def _same(dev, want):
        import torch
        want = torch.device(want)
        return dev.type == want.type and (want.index is None or dev.index == want.index)

    @classmethod
    def _for_device(cls, device):
        import torch
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        ent = cls._by_dev.get(idx)
        if ent is None:
            dev = torch.device("cuda", idx)
            buf = torch.empty(cls.SIZE, dtype=torch.float32, device=dev)
            shadow = None
            # bit-reproducible sums into the arena's slots (csrc/common.h dg_acc_add): a shadow of 128 bytes per float, zero at
            # rest, registered with the library for this device; DUSTY_GAN_DETERMINISTIC=0 keeps the float atomics
            if os.environ.get("DUSTY_GAN_DETERMINISTIC", "1") != "0":
                shadow = torch.zeros(cls.SIZE * 32, dtype=torch.int32, device=dev)   # DG_DET_STRIDE = 128 bytes per slot
                torch.cuda.synchronize(dev)
                with torch.cuda.device(dev):
                    check(lib().dg_det_arena(ptr(buf), cls.SIZE, ptr(shadow)), "dg_det_arena")
            ent = cls._by_dev[idx] = (buf, shadow)
        return ent

    @classmethod
    def begin(cls, device, also=(), draws=(), fetch=None):
        """open a new epoch: the arena - and the fp32 buffers in `also` (the step's gradient buffers) - zero-filled by
        one launch, which also runs the DgDraw jobs in `draws` (the step's parameter draws) and, with `fetch` (a DgFetch),
        fetch_reals of the step's batch"""
        cls.buf, cls.shadow = cls._for_device(device)
        if draws or fetch is not None:
            step_prologue([cls.buf] + list(also), list(draws), fetch)
        else:
            zero_multi([cls.buf] + list(also))
        cls.pos = 0
        cls.epoch += 1

    @classmethod
    def take(cls, n, device=None):
        import torch
        if cls.buf is None or (device is not None and not cls._same(cls.buf.device, device)):
            return None
        a = (cls.pos + 15) // 16 * 16          # 64-byte slices
        if a + n > cls.SIZE:
            return None
        cls.pos = a + n
        return cls.buf[a:a + n]


class CounterQueue:
    """The queued counter advances of one owner (a Trainer; the process-wide default for everything else):
    pending  {counter pointer: [tensor, delta]}
    snap     (counter tensor, src pointer, n, ring pointer, ring slots): filed by the next flush (dg_counter_add_multi_snap)
    ride     the next ParamStore.refresh_transposed carries the pending advances (and the snapshot) in its launch"""
    _all = None   # weak set of every queue (flush_if looks for a counter's queued advance in all of them)

    def __init__(self):
        import weakref
        self.pending, self.snap, self.ride = {}, None, False
        if CounterQueue._all is None:
            CounterQueue._all = weakref.WeakSet()
        CounterQueue._all.add(self)


class _CountersMeta(type):
    """`Counters.pending / .snap / .ride` read and write the CURRENT queue (`Counters.bind`), so the classmethods below and
    their callers are written as for one queue"""
    _STATE = ("pending", "snap", "ride")

    def __getattr__(cls, name):
        if name in _CountersMeta._STATE:
            return getattr(cls._stack[-1], name)
        raise AttributeError(name)

    def __setattr__(cls, name, value):
        if name in _CountersMeta._STATE:
            setattr(cls._stack[-1], name, value)
        else:
            type.__setattr__(cls, name, value)


class Counters(metaclass=_CountersMeta):
    """Device counters (Philox offsets, Adam step counts) are advanced behind their consumers.  The advances of a step are
    queued and applied by ONE kernel at the end of the step (`flush`); anything that reads a counter with a queued
    advance - the next draw from the same generator, `Philox.offset`, the next optimizer step - flushes first.
    The queue is per owner (round-3 review: it was one process-global): a Trainer binds its own `CounterQueue` around its
    public entry points, so the flush / the riding launch at the end of ITS step - possibly being captured into ITS graph -
    never carries advances another trainer of the process has queued."""
    _stack = [CounterQueue()]   # [-1] = the current queue; [0] = the process-wide default

    @classmethod
    def current(cls):
        return cls._stack[-1]

    @classmethod
    def bind(cls, queue):
        """context manager: `queue` is the current queue inside the block"""
        import contextlib

        @contextlib.contextmanager
        def _bound():
            cls._stack.append(queue)
            try:
                yield queue
            finally:
                cls._stack.pop()
        return _bound()

    @classmethod
    def snapshot(cls, ctr, src_ptr, n, ring_ptr, ring):
        """with the next flush - which must advance `ctr` - src[0..n) goes to slot (old ctr) % ring of the ring buffer"""
        cls.snap = (ctr, int(src_ptr), int(n), int(ring_ptr), int(ring))

    @classmethod
    def add(cls, t, n):
        e = cls.pending.setdefault(t.data_ptr(), [t, 0])
        e[1] += int(n)

    @classmethod
    def flush_if(cls, t):
        if t is None:
            return
        if t.data_ptr() in cls.pending:
            cls.flush(mid_step=True)
            return
        for q in list(CounterQueue._all or ()):   # (a counter read outside its owner's entry points)
            if q is not cls._stack[-1] and t.data_ptr() in q.pending:
                with cls.bind(q):
                    cls.flush(mid_step=True)

    @classmethod
    def take_for_ride(cls):
        """(counter pointers, deltas, k, snap_idx, src, n, ring_ptr, ring) of everything pending, for a launch that applies
        them itself (dg_transpose_shadow_multi_tail); None when nothing rides (no flag, nothing pending, more than 8)"""
        import ctypes as C
        if not cls.ride or not cls.pending or len(cls.pending) > 8:
            return None
        cls.ride = False
        items = list(cls.pending.values())
        snap, cls.snap = cls.snap, None
        at = [j for j, (t, _) in enumerate(items) if snap is not None and t.data_ptr() == snap[0].data_ptr()]
        if snap is not None and not at:
            raise RuntimeError("Counters.snapshot: the snapshot's counter has no queued advance")
        cls.pending.clear()
        ptrs = (C.c_void_p * len(items))(*[t.data_ptr() for t, _ in items])
        dels = (C.c_uint64 * len(items))(*[d for _, d in items])
        if snap is None:
            return ptrs, dels, len(items), -1, None, 0, None, 1
        return ptrs, dels, len(items), at[0], snap[1], snap[2], snap[3], snap[4]

    @classmethod
    def flush(cls, mid_step=False):
        """apply everything pending.  mid_step (a consumer needs its counter current while a step with a riding snapshot is
        still running): the snapshot and its counter stay queued - the scalars are not complete yet."""
        import ctypes as C
        held = None
        if mid_step and cls.ride and cls.snap is not None:
            held = cls.pending.pop(cls.snap[0].data_ptr(), None)
        else:
            cls.ride = False
        items = list(cls.pending.values())
        cls.pending.clear()
        if held is not None:
            cls.pending[cls.snap[0].data_ptr()] = held
            snap = None
        else:
            snap, cls.snap = cls.snap, None
        if snap is not None and snap[0].data_ptr() not in [t.data_ptr() for t, _ in items]:
            raise RuntimeError("Counters.snapshot: the snapshot's counter has no queued advance")
        for i in range(0, len(items), 8):
            chunk = items[i:i + 8]
            ptrs = (C.c_void_p * len(chunk))(*[t.data_ptr() for t, _ in chunk])
            dels = (C.c_uint64 * len(chunk))(*[d for _, d in chunk])
            at = [j for j, (t, _) in enumerate(chunk) if snap is not None and t.data_ptr() == snap[0].data_ptr()]
            if at:
                check(lib().dg_counter_add_multi_snap(ptrs, dels, len(chunk), at[0], snap[1], snap[2], snap[3], snap[4],
                                                      stream_ptr()), "dg_counter_add_multi_snap")
            else:
                check(lib().dg_counter_add_multi(ptrs, dels, len(chunk), stream_ptr()), "dg_counter_add_multi")


def tag_sums(t, sums, parts=1):
    """remember on an image tensor the per-sample sums its producer kernel accumulated (DiffAugment's contrast reads them
    instead of making its own pass) - valid while the arena epoch lasts and the tensor is not rewritten.  parts > 1: `sums` is
    [B][parts] partial sums, to be added in index order (dg_step_prologue_fetch)"""
    t._dg_sums = (sums, AccArena.epoch, t._version, int(parts))
    return t


def tagged_sums(t, with_parts=False):
    """the per-sample sums tagged on `t`, or None; with_parts: (sums, parts) - readers that only take one float per sample
    (with_parts=False) see None for a tensor that carries partial sums"""
    tag = getattr(t, "_dg_sums", None)
    if tag is None or tag[1] != AccArena.epoch or tag[2] != t._version:
        return None
    if with_parts:
        return tag[0], tag[3]
    return tag[0] if tag[3] == 1 else None


def policy_mask(policy):
    m = 0
    for p in policy or ():
        if p not in POLICY_BITS:
            raise KeyError(p)
        m |= POLICY_BITS[p]
    return m
