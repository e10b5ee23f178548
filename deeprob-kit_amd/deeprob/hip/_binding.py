"""One ctypes binding of one C header onto one shared object: what ``deeprob.hip`` and its per-library modules are made of.

A header under ``include/`` is the only declaration of its C ABI: the prototypes, the ``DPx_*`` constants and the argument
structs are read from it when a :class:`Binding` is constructed; nothing of them is written down a second time.  The
header is regular C: comments, ``#define NAME value``, ``typedef struct { ... } name;`` and one prototype per ``;``.
"""
import ctypes
import os
import re
import sys
import types

_HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE_DIR = os.path.normpath(os.path.join(_HERE, '..', '..', '..', 'include'))
LIB_DIR = os.path.normpath(os.path.join(_HERE, '..', '..', 'lib'))


class HipError(RuntimeError):
    """Raised when the native library or its header is missing, or a C-ABI call reports a failure."""


_SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint32_t': ctypes.c_uint32,
            'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float, 'double': ctypes.c_double}


def _ctype(decl: str, named: bool, where: str, header: str = 'deeprob_hip.h'):
    """ctypes type of ``[const] type [*...] [name]``: every pointer is a ``c_void_p``, a scalar must be a known word."""
    if '*' in decl:
        return ctypes.c_void_p
    words = re.sub(r'\bconst\b', ' ', decl).split()
    if named and len(words) > 1:
        words = words[:-1]
    if len(words) != 1 or words[0] not in _SCALARS:
        raise HipError("{}: cannot read the type of '{}' in {}".format(header, decl.strip(), where))
    return _SCALARS[words[0]]


def parse_header(text: str, prefix: str = 'dpk', header: str = 'deeprob_hip.h'):
    """``(signatures, constants, structs)`` of a header text: ``{name: (restype, argtypes)}``, ``{DPK_NAME: int}`` and
    ``{struct name: [(field, ctype)]}``.  Raises HipError on anything it does not understand -- it never guesses.
    ``prefix``: what the entry points (lower case) and constants (upper case) of this header begin with; ``header``: its
    name in error messages."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    constants = {}
    for m in re.finditer(r'^#define\s+(' + prefix.upper() + r'_\w+)[ \t]+(.*)$', text, re.M):
        value = re.fullmatch(r'\(?(-?\d+)u?\)?', m.group(2).strip())
        if value is None:
            raise HipError("{}: cannot read the value '{}' of {}".format(header, m.group(2).strip(), m.group(1)))
        constants[m.group(1)] = int(value.group(1))
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    structs = {}
    for m in re.finditer(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', text, re.S):
        fields = []
        for line in filter(None, (l.strip() for l in m.group(1).split(';'))):
            first, *more = line.split(',')
            base = re.sub(r'[\s\*]*\w+\s*$', '', first)          # the type words in front of the first declarator
            for d in [first[len(base):]] + more:
                fields.append((d.replace('*', '').strip(), _ctype(base + ' ' + d, True, 'struct ' + m.group(2), header)))
        structs[m.group(2)] = fields
    text = re.sub(r'typedef\s+struct\s*\w*\s*\{.*?\}\s*\w+\s*;', '', text, flags=re.S)
    text = re.sub(r'extern\s+"C"\s*\{', '', text)
    signatures = {}
    for stmt in filter(None, (s.strip() for s in text.split(';'))):
        if stmt == '}':            # (closes extern "C")
            continue
        m = re.fullmatch(r'(.+?)\b(' + prefix + r'_\w+)\s*\((.*)\)', stmt, re.S)
        if m is None:
            raise HipError("{}: not a prototype: '{}'".format(header, stmt))
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        if '*' in ret:
            if re.sub(r'\s+', ' ', ret).strip() != 'const char *':
                raise HipError("{}: cannot read the return type '{}' of {}".format(header, ret.strip(), name))
            restype = ctypes.c_char_p
        else:
            restype = _ctype(ret, False, name, header)
        argtypes = [] if params == 'void' else [_ctype(p, True, name, header) for p in params.split(',')]
        signatures[name] = (restype, argtypes)
    return signatures, constants, structs


def _view(attr: str):
    return property(lambda module: getattr(module.BINDING, attr), lambda module, value: setattr(module.BINDING, attr, value))


class BoundModule(types.ModuleType):
    """The class of a module built on one :class:`Binding` (its ``BINDING``).  The names under which callers and tests
    have always reached the paths, the handle and the minimum ABI version stay, as views of the binding: reading
    ``module.LIB_PATH`` reads ``BINDING.lib_path``, assigning to it (``monkeypatch.setattr`` included) assigns there.
    There is no second copy that could stop being read.  A module adopts the class with :func:`bound_module`."""
    LIB_PATH = _view('lib_path')
    HEADER_PATH = _view('header_path')
    ABI_VERSION = _view('min_abi')
    _lib = _view('lib')


def bound_module(name: str):
    """``bound_module(__name__)``, after the module has set its ``BINDING``."""
    sys.modules[name].__class__ = BoundModule


class Binding:
    """``include/deeprob_<name>.h`` (prefix ``<prefix>_``) bound onto ``lib/libdeeprob_<name>.so``.

    The paths and the loaded handle live here and nowhere else: ``header_path``, ``lib_path``, ``lib`` (None until
    :meth:`load`).  What differs between the libraries is an argument:

    ``min_abi``          the oldest ``<prefix>_abi_version()`` that loads (an older library asks to be rebuilt);
    ``env``              an environment variable that overrides ``lib_path`` -- measurement builds of an older ABI (A/B
                         runs): under it, what exists is bound and a missing symbol is skipped;
    ``onto``             another binding: this header declares further entry points of THAT binding's library and is bound
                         onto its handle;
    ``not_implemented``  the name of the status constant that raises ``NotImplementedError`` instead of ``HipError``."""

    def __init__(self, name: str, prefix: str, min_abi: int = 0, env: str = None, onto: 'Binding' = None,
                 not_implemented: str = None):
        self.name, self.prefix, self.min_abi, self.env, self.onto = name, prefix, min_abi, env, onto
        self.header_path = os.path.join(INCLUDE_DIR, 'deeprob_{}.h'.format(name))
        self.lib_path = os.path.join(LIB_DIR, 'libdeeprob_{}.so'.format(name)) if onto is None else onto.lib_path
        if env is not None:
            self.lib_path = os.environ.get(env, self.lib_path)
        self.lib = None                  # (with ``onto``: that binding's handle once this header is bound onto it)
        self.signatures, self.constants, self.structs = self.read_header()
        self.not_implemented = None if not_implemented is None else self.constants[not_implemented]

    def read_header(self):
        header = 'deeprob_{}.h'.format(self.name)
        if not os.path.isfile(self.header_path):
            raise HipError("{} not found at {} -- it is the declaration of the C ABI this binding is built "
                           "from".format(header, self.header_path))
        with open(self.header_path) as f:
            return parse_header(f.read(), prefix=self.prefix, header=header)

    def struct(self, c_name: str, doc: str = None):
        """The ctypes mirror of the header's ``typedef struct { ... } c_name;``."""
        return type(c_name, (ctypes.Structure,), {'_fields_': self.structs[c_name], '__doc__': doc})

    def load(self):
        """Load the library (built in-tree by ``__graft_entry__.build()``) and bind every symbol of the header."""
        if self.onto is not None:
            lib = self.onto.load()
            if self.lib is None:
                self.lib = self._bind(lib)
            return lib
        if self.lib is None:
            so = 'libdeeprob_{}.so'.format(self.name)
            if not os.path.isfile(self.lib_path):
                raise HipError(
                    "{} not found at {} -- build it with `make -C deeprob-kit_amd/csrc` "
                    "(or __graft_entry__.build()); there is no CPU fallback".format(so, self.lib_path))
            lib = ctypes.CDLL(self.lib_path)
            if self.min_abi:
                abi = self.prefix + '_abi_version'
                version = getattr(lib, abi)() if hasattr(lib, abi) else 0
                if version < self.min_abi:
                    raise HipError(
                        "{} at {} has ABI version {}, this binding needs {} -- rebuild it with `make -C "
                        "deeprob-kit_amd/csrc` (or __graft_entry__.build())".format(so, self.lib_path, version, self.min_abi))
            self.lib = self._bind(lib)
        return self.lib

    def _bind(self, lib):
        for name, (restype, argtypes) in self.signatures.items():
            try:
                fn = getattr(lib, name)  # AttributeError if the .so and the header disagree
            except AttributeError:
                if self.env is not None and self.env in os.environ:
                    continue
                raise
            fn.restype = restype
            fn.argtypes = argtypes
        return lib

    def abi_version(self) -> int:
        """``<prefix>_abi_version()`` of the loaded library."""
        return getattr(self.load(), self.prefix + '_abi_version')()

    def check(self, rc: int, fn):
        """Raise ``HipError("<name> failed (<rc>): <last error>")`` for the negative result ``rc`` of entry point ``fn``."""
        if rc < 0:
            msg = getattr(self.load(), self.prefix + '_last_error')()
            text = "{} failed ({}): {}".format(fn.__name__, rc, msg.decode() if msg else '')
            raise (NotImplementedError if rc == self.not_implemented else HipError)(text)

    def call(self, fn, *args) -> int:
        """``fn(*args)`` for an entry point that returns a status or a ``*_workspace_bytes`` size: the (non-negative)
        result, HipError on a negative one."""
        rc = fn(*args)
        if rc < 0:
            self.check(rc, fn)
        return rc
