"""TEST INFRASTRUCTURE: the CPU build of the engine behind the Python binding (tests/test_engine_cpu_host.py).

csrc/engine.hip compiles as host C++ against the HIP stand-in of tests/native/hipcpu and is linked into
tests/native/engine_cpu_driver.cpp, a program that makes the C-ABI calls of a call list.  A sanitized program cannot be
loaded into Python, so `Session` stands where the ctypes library stands (sgfhe_jl_amd._lib.lib()): every call the
binding makes is written as one record of the list into the pipe of a running sanitized driver, and the record the driver
answers with -- status, text, every buffer -- is copied back into the caller's arrays.  Engine, Circuit and the helpers
of the GPU tests therefore run unchanged, and compare with their references as they go.  The list is kept, and
`Session.finish()` runs it again from the file, sanitized under the other fill byte and in the plain build: all three
outputs must be the same bytes.

Why a live session and not a list written ahead: most calls of the binding depend on what an earlier call returned (a
count queried before a buffer is sized, kernel names held to a table before the next call, a reference computed from a
returned array), and the GPU tests' own functions, cases and references can then be used as they are instead of being
restated.  The price is the marshalling below: it reads an argument the way ctypes would -- an int, None, bytes, a
ctypes object or byref() of one, or a c_void_p that numpy's `ndarray.ctypes.data_as` made (numpy keeps the array on it as
`_arr`, which is how the buffer's size is known).  A bare `c_void_p(address)` carries no size: its array must have been
named with `Session.register` first (`device=True`: the driver puts it into memory of hipMalloc).  Anything else is
refused with an assertion, never guessed.
"""

import ctypes
import os
import shutil
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("SGFHE_CPU_CLANG") or "/opt/rocm/lib/llvm/bin/clang++"
SAN_FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
PLAIN_FLAGS = ["-O2"]
FILLS = ("0x00", "0xA5")
BUILD_TIMEOUT, RUN_TIMEOUT = 300, 600

_HANDLE_BASE = 0x5CF0000000          # handles as Python sees them: this + 16 id; the driver keeps the pointers
_MAKERS = ("sgfhe_ctx_create", "sgfhe_ctx_clone", "sgfhe_circuit_create")
_TEXT = ("sgfhe_version", "sgfhe_build_id", "sgfhe_last_error_string")


def build_command(exe, flags):
    """The one command that builds a driver (DESIGN.md section 2 quotes the plain form for gdb)."""
    nat = os.path.join(ROOT, "tests", "native")
    return [CLANG, "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Werror"] + flags + [
        "-I", os.path.join(nat, "hipcpu"), '-DSGFHE_BUILD_ID="cpu"',
        os.path.join(nat, "engine_cpu_driver.cpp"), os.path.join(nat, "hipcpu", "hipcpu.cpp"),
        "-x", "c++", os.path.join(ROOT, "sgfhe.jl_amd", "csrc", "engine.hip"), "-o", exe]


def build(exe, flags):
    """-> None, or the reason the driver cannot be built here (no compiler, no sanitizer runtimes)."""
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        return "no ROCm clang++ (%s)" % CLANG
    b = subprocess.run(build_command(exe, flags), capture_output=True, text=True, timeout=BUILD_TIMEOUT)
    if b.returncode != 0 and "sanitize" in b.stderr and ("cannot find" in b.stderr or "no such file" in b.stderr.lower()):
        return "the sanitizer runtimes are not installed: " + b.stderr[-300:]
    assert b.returncode == 0, b.stderr[-4000:]
    return None


def run_env(fill, launch_log=None):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1",
               HIPCPU_FILL=fill)
    env.pop("LD_PRELOAD", None)
    if launch_log:
        env["HIPCPU_LAUNCH_LOG"] = launch_log
    return env


class DriverDied(AssertionError):
    pass


class Session:
    """One running sanitized driver, shaped like the ctypes library: `Session.sgfhe_x(*args)` makes the call."""

    def __init__(self, san_exe, plain_exe, workdir, name):
        self.san_exe, self.plain_exe, self.name = san_exe, plain_exe, name
        self.base = os.path.join(str(workdir), name)
        self.list_path, self.out_path = self.base + ".list", self.base + ".out0"
        self.launch_log = self.base + ".launches"
        self._list = open(self.list_path, "wb")
        self._out = open(self.out_path, "wb")
        self._err = open(self.base + ".err0", "wb")
        self.proc = subprocess.Popen([san_exe, "/dev/stdin", "/dev/stdout"], stdin=subprocess.PIPE,
                                     stdout=subprocess.PIPE, stderr=self._err,
                                     env=run_env(FILLS[0], self.launch_log))
        self._next_id = 1
        self.live = {}                 # id -> "ctx" | "circuit"
        self.known = {}                # address -> (array, device) of Session.register
        self.calls = 0
        self.closed = False
        self._send(b"SGCL")
        self._keep(self._read(4))

    # ---- the pipe ---------------------------------------------------------------------------------------------------
    def _send(self, data):
        self._list.write(data)
        try:
            self.proc.stdin.write(data)
            self.proc.stdin.flush()
        except (BrokenPipeError, OSError):
            self._died()

    def _keep(self, data):
        self._out.write(data)
        return data

    def _read(self, n):
        data = self.proc.stdout.read(n) if n else b""
        if len(data) != n:
            self._died()
        return data

    def _died(self):
        self.closed = True
        try:
            self.proc.stdin.close()
        except OSError:
            pass
        rc = self.proc.wait(timeout=60)
        self._err.flush()
        with open(self.base + ".err0", "r", errors="replace") as fh:
            err = fh.read()
        raise DriverDied("%s: the sanitized driver ended with status %s after %d calls\n%s"
                         % (self.name, rc, self.calls, err[-6000:]))

    def register(self, arr, device=False):
        """Name the array behind bare pointers (c_void_p(arr.ctypes.data), or that address as an int) of later calls.
        While an array is registered, an integer argument equal to its address is taken for the pointer: register for
        the calls that need it and clear `known` after them (addresses lie far above any count, flag or shape here)."""
        assert arr.flags["C_CONTIGUOUS"] and arr.ctypes.data >= 1 << 32
        self.known[arr.ctypes.data] = (arr, device)
        return arr.ctypes.data

    def _known(self, value):
        arr, device = self.known[value]
        n, addr = arr.nbytes, arr.ctypes.data
        return (struct.pack("<BQ", 5 if device else 1, n) + ctypes.string_at(addr, n),
                (lambda data: ctypes.memmove(addr, data, n)))

    # ---- one call -----------------------------------------------------------------------------------------------------
    def __getattr__(self, name):
        if not name.startswith("sgfhe_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _handle_id(self, value):
        if value is None:
            return None
        k = value - _HANDLE_BASE
        return k // 16 if k > 0 and k % 16 == 0 and k // 16 in self.live else None

    def _arg(self, name, a, last):
        """-> (record bytes, sink): sink(bytes) copies a returned buffer back, None for an argument without one."""
        if a is None:
            return b"\x02", None
        if isinstance(a, (bool, int)):
            if int(a) in self.known:
                return self._known(int(a))
            hid = self._handle_id(int(a))
            return (struct.pack("<BI", 3, hid), None) if hid else (struct.pack("<Bq", 0, int(a)), None)
        if isinstance(a, (bytes, bytearray)):
            return struct.pack("<BQ", 1, len(a)) + bytes(a), (lambda data: None)
        arr = getattr(a, "_arr", None)
        if arr is not None:            # numpy's ndarray.ctypes.data_as keeps the array on the pointer
            assert arr.flags["C_CONTIGUOUS"], "a pointer into an array that is not contiguous"
            n, addr = arr.nbytes, arr.ctypes.data
            return struct.pack("<BQ", 1, n) + ctypes.string_at(addr, n), (lambda data: ctypes.memmove(addr, data, n))
        if type(a).__name__ == "CArgObject":      # ctypes.byref(x)
            obj = a._obj
            if last and name.startswith(_MAKERS) and isinstance(obj, ctypes.c_void_p):
                hid = self._next_id
                self._next_id += 1
                self.live[hid] = "ctx" if name.startswith("sgfhe_ctx_") else "circuit"
                obj.value = _HANDLE_BASE + 16 * hid
                return struct.pack("<BI", 4, hid), None
            a = obj
        elif isinstance(a, ctypes.c_void_p):
            if a.value is None:
                return b"\x02", None
            if a.value in self.known:
                return self._known(a.value)
            hid = self._handle_id(a.value)
            assert hid, "%s: a raw pointer argument (%#x) that is no handle of this session" % (name, a.value)
            return struct.pack("<BI", 3, hid), None
        elif isinstance(a, ctypes._SimpleCData):
            return struct.pack("<Bq", 0, int(a.value)), None
        assert isinstance(a, (ctypes.Array, ctypes.Structure, ctypes._SimpleCData)), (name, type(a))
        n, addr = ctypes.sizeof(a), ctypes.addressof(a)
        return struct.pack("<BQ", 1, n) + ctypes.string_at(addr, n), (lambda data: ctypes.memmove(addr, data, n))

    def _call(self, name, args):
        if self.closed:
            if name.endswith("_destroy"):
                return 0               # a finalizer after the session: the driver destroyed what was left
            raise DriverDied("%s: %s after the session ended" % (self.name, name))
        parts, sinks = [], []
        for i, a in enumerate(args):
            rec, sink = self._arg(name, a, i == len(args) - 1)
            parts.append(rec)
            if sink is not None:
                sinks.append(sink)
        nb = name.encode()
        self._send(struct.pack("<H", len(nb)) + nb + struct.pack("<I", len(args)) + b"".join(parts))
        value, tl = struct.unpack("<qI", self._keep(self._read(12)))
        text = self._keep(self._read(tl))
        for sink in sinks:
            n, = struct.unpack("<Q", self._keep(self._read(8)))
            sink(self._keep(self._read(n)))
        self.calls += 1
        if name.endswith("_destroy") and value == 0:
            hid = self._handle_id(args[0].value if isinstance(args[0], ctypes.c_void_p) else args[0])
            self.live.pop(hid, None)
        if name == "sgfhe_last_error_string":
            return text
        if value != 0:
            self.last_text = text
        return text if name in _TEXT else value

    # ---- the end ----------------------------------------------------------------------------------------------------
    def finish(self):
        """Destroy what is left (circuits, then ctxs), end the sanitized driver (LeakSanitizer reports at its exit), run
        the list again under the other fill byte and in the plain build, and hold all three outputs to the same bytes.
        -> {kernel name: launches} of the first run."""
        for kind in ("circuit", "ctx"):
            for hid in sorted((h for h, k in self.live.items() if k == kind), reverse=True):
                rc = self._call("sgfhe_%s_destroy" % kind, (ctypes.c_void_p(_HANDLE_BASE + 16 * hid),))
                assert rc == 0, (kind, hid, rc)
        self.closed = True
        self.proc.stdin.close()
        rest = self.proc.stdout.read()
        rc = self.proc.wait(timeout=RUN_TIMEOUT)
        for fh in (self._list, self._out, self._err):
            fh.close()
        with open(self.base + ".err0", "r", errors="replace") as fh:
            err = fh.read()
        assert rc == 0 and not rest, "%s: sanitized run, status %s\n%s" % (self.name, rc, err[-6000:])
        with open(self.out_path, "rb") as fh:
            first = fh.read()
        for tag, exe, fill in (("sanitized, fill " + FILLS[1], self.san_exe, FILLS[1]), ("plain", self.plain_exe, FILLS[1])):
            out = self.base + (".out1" if exe is self.san_exe else ".out2")
            r = subprocess.run([exe, self.list_path, out], capture_output=True, text=True, timeout=RUN_TIMEOUT,
                               env=run_env(fill))
            assert r.returncode == 0, "%s: %s run, status %s\n%s" % (self.name, tag, r.returncode, r.stderr[-6000:])
            with open(out, "rb") as fh:
                other = fh.read()
            assert other == first, "%s: the %s run differs from the sanitized run under fill %s (%s)" % (
                self.name, tag, FILLS[0], _first_difference(first, other))
            os.remove(out)
        launches = {}
        with open(self.launch_log) as fh:
            for line in fh:
                k, n, _oob = line.split()
                launches[k] = int(n)
        os.remove(self.list_path)
        os.remove(self.out_path)
        return launches


def _first_difference(a, b):
    if len(a) != len(b):
        return "lengths %d and %d" % (len(a), len(b))
    i = next(i for i in range(len(a)) if a[i] != b[i])
    return "first at byte %d of %d" % (i, len(a))
