"""Expression vocabulary for Map and Filter (K13).

``bs.col(i)`` and Python scalars combine through the usual operators into
``Expr`` trees.  A Map/Filter chain written with them runs as ONE HIP
kernel launch per batch on a GPU session (csrc/expr.hip), and as ordinary
torch ops everywhere else.  Python-callable UDFs are untouched; nothing is
auto-traced.

Semantics are defined by torch: ``Expr.eval(cols)`` applies the tree with
plain torch ops and is both the CPU path and the oracle.  ``Expr.dtype``
is inferred by applying the same ops to empty tensors, so promotion is
torch's own (an int64 column against a Python float computes in float32).
Integer arithmetic wraps.  A float->int cast of NaN or an out-of-range
value is unspecified.

``//`` and ``%`` take a positive integer literal divisor and an integer
(or bool) dividend, and ``<<``/``>>`` a literal amount in [0, bits): every
expression is total, no row can fault, so predicates and maps compose in
any order.

Three layers live here:
  * ``Expr`` (construction, typing, eval, substitution);
  * ``compile_program``: a flat, typed, register-based bytecode with
    shared subexpressions and liveness-allocated registers, plus
    ``run_program_host``, a torch interpreter of the same bytecode that
    verifies the lowering without a GPU;
  * ``ExprSpec``/``ExprReader``: the reader that Map/Filter hand out, and
    that downstream expression ops fold themselves into.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .frame import Frame
from .schema import BYTES, OBJECT, Schema
from .sliceio import Reader

# Element dtypes of the vocabulary; the index is the wire dtype code.
DTYPES = (torch.bool, torch.int32, torch.int64, torch.float32,
          torch.float64)
_DT_CODE = {dt: i for i, dt in enumerate(DTYPES)}
_DT_BOOL, _DT_I32, _DT_I64, _DT_F32, _DT_F64 = range(5)

# Native-eligibility limits (mirrored by csrc/expr.hip, which re-checks).
MAX_REGS = 16
MAX_INSTRS = 48
MAX_INPUTS = 4
MAX_OUTPUTS = 4

# Opcodes (csrc/expr.hip holds the same list).
(OP_CONST, OP_LOAD, OP_CAST, OP_ADD, OP_SUB, OP_MUL, OP_NEG, OP_ABS,
 OP_DIV, OP_FLOORDIV, OP_MOD, OP_AND, OP_OR, OP_XOR, OP_NOT, OP_SHL,
 OP_SHR, OP_EQ, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE, OP_WHERE, OP_MIN,
 OP_MAX) = range(26)
NUM_OPS = 26
FLAG_B_IMM = 1

_BINARY = {"add": OP_ADD, "sub": OP_SUB, "mul": OP_MUL, "truediv": OP_DIV,
           "and": OP_AND, "or": OP_OR, "xor": OP_XOR, "min": OP_MIN,
           "max": OP_MAX}
_COMPARE = {"eq": OP_EQ, "ne": OP_NE, "lt": OP_LT, "le": OP_LE,
            "gt": OP_GT, "ge": OP_GE}
_UNARY = {"neg": OP_NEG, "abs": OP_ABS, "not": OP_NOT}
# literal-first forms that may swap operands (torch swaps them the same
# way: ``3 + x`` is ``x.__radd__(3)``); min/max keep their order, which
# decides the NaN that propagates
_COMMUTE = {OP_ADD, OP_MUL, OP_AND, OP_OR, OP_XOR, OP_EQ, OP_NE}
_FLIP = {OP_LT: OP_GT, OP_GT: OP_LT, OP_LE: OP_GE, OP_GE: OP_LE}


def _is_lit(v) -> bool:
    return isinstance(v, (bool, int, float))


def _apply(op: str, a: list, aux):
    """One node in torch ops.  Operands are tensors or Python scalars;
    this single function is eval, the dtype inference and the host
    interpreter's arithmetic."""
    if op == "add":
        return a[0] + a[1]
    if op == "sub":
        return a[0] - a[1]
    if op == "mul":
        return a[0] * a[1]
    if op == "truediv":
        if not isinstance(a[0], torch.Tensor):
            # scalar / tensor: torch spells it reciprocal() * scalar,
            # which rounds twice; divide for real
            dt = torch.result_type(a[0], a[1])
            return torch.tensor(a[0], dtype=dt, device=a[1].device) / a[1]
        return a[0] / a[1]
    if op == "floordiv":
        return a[0] // a[1]
    if op == "mod":
        return a[0] % a[1]
    if op == "and":
        return a[0] & a[1]
    if op == "or":
        return a[0] | a[1]
    if op == "xor":
        return a[0] ^ a[1]
    if op == "lshift":
        return a[0] << a[1]
    if op == "rshift":
        return a[0] >> a[1]
    if op == "eq":
        return a[0] == a[1]
    if op == "ne":
        return a[0] != a[1]
    if op == "lt":
        return a[0] < a[1]
    if op == "le":
        return a[0] <= a[1]
    if op == "gt":
        return a[0] > a[1]
    if op == "ge":
        return a[0] >= a[1]
    if op == "neg":
        return -a[0]
    if op == "abs":
        return torch.abs(a[0])
    if op == "not":
        return ~a[0]
    if op == "to":
        return a[0].to(aux)
    if op == "where":
        return torch.where(a[0], a[1], a[2])
    if op in ("min", "max"):
        # torch.minimum wants tensors: a literal joins at the dtype
        # torch.result_type gives the pair, like every other operator
        t = a[0] if isinstance(a[0], torch.Tensor) else a[1]
        dt = torch.result_type(a[0], a[1])
        x, y = (v.to(dt) if isinstance(v, torch.Tensor)
                else torch.tensor(v, dtype=dt, device=t.device)
                for v in a)
        return torch.minimum(x, y) if op == "min" else torch.maximum(x, y)
    raise AssertionError(op)


class Expr:
    """A node of an expression tree.  ``dtype`` is None until every
    column below it is typed (``col(i, dtype)`` or ``bind(schema)``)."""

    __slots__ = ("op", "args", "aux", "dtype", "_key")

    def __init__(self, op: str, args: tuple = (), aux=None):
        self.op = op
        self.args = args
        self.aux = aux
        self.dtype = None
        self._key = None
        self._check_and_type()

    # -- typing ------------------------------------------------------------

    def _check_and_type(self):
        op, args = self.op, self.args
        if op == "col":
            self.dtype = self.aux[1]
            return
        if op in ("floordiv", "mod"):
            d = args[1]
            if isinstance(d, bool) or not isinstance(d, int) or d <= 0 \
                    or isinstance(args[0], (bool, int, float)):
                raise TypeError(
                    f"{'//' if op == 'floordiv' else '%'} takes an Expr "
                    "dividend and a positive integer literal divisor")
        if op in ("lshift", "rshift"):
            s = args[1]
            if isinstance(s, bool) or not isinstance(s, int) \
                    or not isinstance(args[0], Expr):
                raise TypeError("shift takes an Expr and an integer "
                                "literal amount")
        sub = [a for a in args if isinstance(a, Expr)]
        for a in sub:
            if a.dtype in (BYTES, OBJECT):
                raise TypeError(
                    f"a {a.dtype.upper()} column may only pass through "
                    "a Map unchanged; it cannot take part in an "
                    "expression")
        if any(a.dtype is None for a in sub):
            return  # typed later, by bind()
        if op in ("floordiv", "mod") and args[0].dtype.is_floating_point:
            raise TypeError("// and % take an integer dividend")
        if op in ("lshift", "rshift"):
            dt = args[0].dtype
            if dt not in (torch.int32, torch.int64):
                raise TypeError("shift takes an int32 or int64 operand")
            bits = 32 if dt == torch.int32 else 64
            if not (0 <= args[1] < bits):
                raise TypeError(
                    f"shift amount {args[1]} outside [0, {bits})")
        if op == "where" and args[0].dtype != torch.bool:
            raise TypeError("where() takes a bool condition")
        try:
            probe = [torch.empty(0, dtype=a.dtype) if isinstance(a, Expr)
                     else a for a in args]
            dt = _apply(op, probe, self.aux).dtype
        except (RuntimeError, NotImplementedError) as e:
            raise TypeError(f"{op}: {e}") from None
        if dt not in _DT_CODE:
            raise TypeError(f"{op}: result dtype {dt} is outside the "
                            "expression vocabulary")
        self.dtype = dt

    def bind(self, schema: Schema) -> "Expr":
        """The same tree with every column typed from ``schema``."""
        if self.op == "col":
            i = self.aux[0]
            if not (0 <= i < schema.num_columns):
                raise TypeError(
                    f"col({i}) out of range for {schema!r}")
            dt = schema.dtypes[i]
            if self.dtype is not None and self.dtype != dt:
                raise TypeError(
                    f"col({i}) declared {self.dtype}, schema has {dt}")
            if dt not in _DT_CODE and dt not in (BYTES, OBJECT):
                raise TypeError(
                    f"col({i}): dtype {dt} is outside the expression "
                    "vocabulary")
            return Expr("col", (), (i, dt))
        return Expr(self.op,
                    tuple(a.bind(schema) if isinstance(a, Expr) else a
                          for a in self.args), self.aux)

    def substitute(self, cols: Sequence["Expr"]) -> "Expr":
        """Replace col(i) by cols[i] (composition of two stages)."""
        if self.op == "col":
            return cols[self.aux[0]]
        return Expr(self.op,
                    tuple(a.substitute(cols) if isinstance(a, Expr) else a
                          for a in self.args), self.aux)

    def key(self) -> tuple:
        """Structural identity (shared-subexpression detection)."""
        if self._key is None:
            self._key = (self.op, self.aux) + tuple(
                a.key() if isinstance(a, Expr) else (type(a).__name__, a)
                for a in self.args)
        return self._key

    def columns(self) -> set:
        if self.op == "col":
            return {self.aux[0]}
        out = set()
        for a in self.args:
            if isinstance(a, Expr):
                out |= a.columns()
        return out

    # -- evaluation --------------------------------------------------------

    def eval(self, cols: Sequence):
        """Evaluate with ordinary torch ops over a column list."""
        memo: Dict[tuple, object] = {}

        def go(e):
            if not isinstance(e, Expr):
                return e
            k = e.key()
            if k not in memo:
                if e.op == "col":
                    memo[k] = cols[e.aux[0]]
                else:
                    memo[k] = _apply(e.op, [go(a) for a in e.args], e.aux)
            return memo[k]
        return go(self)

    # -- operators ---------------------------------------------------------

    @staticmethod
    def _operand(v):
        if isinstance(v, Expr) or _is_lit(v):
            return v
        return None

    def _bin(self, op, other, swap=False):
        o = Expr._operand(other)
        if o is None:
            if op in ("floordiv", "mod", "lshift", "rshift"):
                raise TypeError(f"{op}: unsupported operand {other!r}")
            return NotImplemented
        return Expr(op, (o, self) if swap else (self, o))

    def __add__(self, o): return self._bin("add", o)
    def __radd__(self, o): return self._bin("add", o, True)
    def __sub__(self, o): return self._bin("sub", o)
    def __rsub__(self, o): return self._bin("sub", o, True)
    def __mul__(self, o): return self._bin("mul", o)
    def __rmul__(self, o): return self._bin("mul", o, True)
    def __truediv__(self, o): return self._bin("truediv", o)
    def __rtruediv__(self, o): return self._bin("truediv", o, True)
    def __floordiv__(self, o): return self._bin("floordiv", o)
    def __rfloordiv__(self, o): return self._bin("floordiv", o, True)
    def __mod__(self, o): return self._bin("mod", o)
    def __rmod__(self, o): return self._bin("mod", o, True)
    def __and__(self, o): return self._bin("and", o)
    def __rand__(self, o): return self._bin("and", o, True)
    def __or__(self, o): return self._bin("or", o)
    def __ror__(self, o): return self._bin("or", o, True)
    def __xor__(self, o): return self._bin("xor", o)
    def __rxor__(self, o): return self._bin("xor", o, True)
    def __lshift__(self, o): return self._bin("lshift", o)
    def __rlshift__(self, o): return self._bin("lshift", o, True)
    def __rshift__(self, o): return self._bin("rshift", o)
    def __rrshift__(self, o): return self._bin("rshift", o, True)
    def __eq__(self, o): return self._bin("eq", o)  # type: ignore
    def __ne__(self, o): return self._bin("ne", o)  # type: ignore
    def __lt__(self, o): return self._bin("lt", o)
    def __le__(self, o): return self._bin("le", o)
    def __gt__(self, o): return self._bin("gt", o)
    def __ge__(self, o): return self._bin("ge", o)
    def __neg__(self): return Expr("neg", (self,))
    def __abs__(self): return Expr("abs", (self,))
    def __invert__(self): return Expr("not", (self,))
    __hash__ = None  # type: ignore  (== builds a node)

    def __bool__(self):
        raise TypeError("an Expr has no truth value; combine predicates "
                        "with & | ~")

    def abs(self) -> "Expr":
        return Expr("abs", (self,))

    def to(self, dtype) -> "Expr":
        if dtype not in _DT_CODE:
            raise TypeError(f"to({dtype}): outside the expression "
                            "vocabulary")
        return Expr("to", (self,), dtype)

    def __repr__(self):
        if self.op == "col":
            return f"col({self.aux[0]})"
        body = ", ".join(repr(a) for a in self.args)
        return f"{self.op}({body}{', ' + str(self.aux) if self.aux else ''})"


def col(i: int, dtype=None) -> Expr:
    """Input column ``i``.  ``dtype`` is optional: Map/Filter type the
    column from their dep's schema."""
    if isinstance(i, bool) or not isinstance(i, int) or i < 0:
        raise TypeError(f"col index must be a non-negative int, got {i!r}")
    return Expr("col", (), (i, dtype))


def _need_expr(fn, *vals):
    if not any(isinstance(v, Expr) for v in vals):
        raise TypeError(f"{fn}() needs at least one Expr operand")
    for v in vals:
        if not isinstance(v, Expr) and not _is_lit(v):
            raise TypeError(f"{fn}(): unsupported operand {v!r}")


def where(c, a, b) -> Expr:
    if not isinstance(c, Expr):
        raise TypeError("where() takes an Expr condition")
    _need_expr("where", c, a, b)
    return Expr("where", (c, a, b))


def minimum(a, b) -> Expr:
    _need_expr("minimum", a, b)
    return Expr("min", (a, b))


def maximum(a, b) -> Expr:
    _need_expr("maximum", a, b)
    return Expr("max", (a, b))


def is_exprs(fn) -> bool:
    """True when a Map/Filter argument is written in the vocabulary."""
    if isinstance(fn, Expr):
        return True
    if isinstance(fn, (tuple, list)) and any(isinstance(e, Expr)
                                             for e in fn):
        if not all(isinstance(e, Expr) for e in fn):
            raise TypeError("a Map output list mixes Exprs with other "
                            "values; every output must be an Expr")
        return True
    return False


# -- program form -----------------------------------------------------------

def _imm_bits(v, code: int) -> int:
    """A literal as the signed 64-bit image of its register slot."""
    import struct
    if code == _DT_F64:
        return struct.unpack("<q", struct.pack("<d", float(v)))[0]
    if code == _DT_F32:
        f = torch.tensor(float(v), dtype=torch.float32)
        return int(f.view(torch.int32).item()) & 0xFFFFFFFF
    if code == _DT_BOOL:
        return int(bool(v))
    bits = 32 if code == _DT_I32 else 64
    x = int(v) & ((1 << bits) - 1)
    if x >= 1 << (bits - 1):
        x -= 1 << bits
    return x


class Program:
    """Flat bytecode for one (outputs, predicate) pair.

    ``instrs`` holds the predicate section ``[0, n_pred)`` followed by the
    output section ``[n_pred, len)``; each section allocates registers on
    its own, so the kernel can count with the first and write with the
    second.  An instruction is ``(op, dt, dst, a, b, c, flags, imm)``:
    ``dt`` is the compute dtype code, ``a``/``b``/``c`` are registers
    (``a`` is the input slot for LOAD, ``c`` the source dtype for CAST),
    and ``imm`` replaces ``b`` when ``flags & FLAG_B_IMM``.

    ``outputs[i]`` is ``("reg", r)`` or, for a bare column of a
    predicate-free program, ``("col", input_column)``: returned as is.
    """

    def __init__(self):
        self.instrs: List[tuple] = []
        self.n_pred = 0
        self.pred_reg = -1
        self.inputs: List[int] = []       # input slot -> frame column
        self.in_dtypes: List = []
        self.outputs: List[tuple] = []
        self.out_dtypes: List = []
        self.nregs = 0
        self.eligible = True
        self.reason = ""
        self._code = None

    def code(self) -> torch.Tensor:
        """[n, 2] int64 host tensor: packed fields, immediate."""
        if self._code is None:
            rows = []
            for op, dt, dst, a, b, c, flags, imm in self.instrs:
                w = (op | dt << 8 | dst << 16 | a << 24 | b << 32
                     | c << 40 | flags << 48)
                rows.append([w, imm])
            self._code = torch.tensor(rows, dtype=torch.int64).reshape(
                len(rows), 2)
        return self._code


class _Lower:
    """One section: Expr DAG -> SSA values -> registers."""

    def __init__(self, slot_of: Dict[int, int]):
        self.slot_of = slot_of
        self.vals: List[tuple] = []   # (op, dt, (srcs), c, flags, imm)
        self.memo: Dict[tuple, int] = {}

    def emit(self, key, op, dt, srcs=(), c=0, flags=0, imm=0) -> int:
        if key in self.memo:
            return self.memo[key]
        self.vals.append((op, dt, tuple(srcs), c, flags, imm))
        self.memo[key] = len(self.vals) - 1
        return self.memo[key]

    def const(self, v, code) -> int:
        imm = _imm_bits(v, code)
        return self.emit(("const", code, imm), OP_CONST, code, imm=imm)

    def cast(self, vid: int, src, dst) -> int:
        if src == dst:
            return vid
        return self.emit(("cast", vid, dst), OP_CAST, _DT_CODE[dst],
                         (vid,), c=_DT_CODE[src])

    def operand(self, a, dt) -> int:
        """An operand as a value of dtype ``dt``."""
        if isinstance(a, Expr):
            return self.cast(self.lower(a), a.dtype, dt)
        return self.const(a, _DT_CODE[dt])

    def binary(self, opc, dt, x, y) -> int:
        """x, y: Expr or literal, computed at dtype ``dt``; a literal
        rides as the immediate of operand b where the opcode allows."""
        code = _DT_CODE[dt]
        if not isinstance(x, Expr) and isinstance(y, Expr):
            if opc in _COMMUTE:
                x, y = y, x
            elif opc in _FLIP:
                x, y, opc = y, x, _FLIP[opc]
        xv = self.operand(x, dt)
        if not isinstance(y, Expr):
            imm = _imm_bits(y, code)
            return self.emit((opc, code, xv, "imm", imm), opc, code,
                             (xv,), flags=FLAG_B_IMM, imm=imm)
        yv = self.operand(y, dt)
        return self.emit((opc, code, xv, yv), opc, code, (xv, yv))

    def lower(self, e: Expr) -> int:
        k = ("expr",) + e.key()
        if k in self.memo:
            return self.memo[k]
        v = self._lower(e)
        self.memo[k] = v
        return v

    def _lower(self, e: Expr) -> int:
        op, args = e.op, e.args
        if op == "col":
            code = _DT_CODE[e.dtype]
            return self.emit(("load", e.aux[0]), OP_LOAD, code,
                             c=self.slot_of[e.aux[0]])
        if op == "to":
            return self.cast(self.lower(args[0]), args[0].dtype, e.aux)
        if op in _UNARY:
            opc, code = _UNARY[op], _DT_CODE[e.dtype]
            xv = self.cast(self.lower(args[0]), args[0].dtype, e.dtype)
            return self.emit((opc, code, xv), opc, code, (xv,))
        if op in _COMPARE:
            probe = [torch.empty(0, dtype=a.dtype) if isinstance(a, Expr)
                     else a for a in args]
            return self.binary(_COMPARE[op], torch.result_type(*probe),
                               args[0], args[1])
        if op in _BINARY:
            opc = _BINARY[op]
            if e.dtype == torch.bool and opc in (OP_ADD, OP_MUL):
                # torch: bool+bool is OR, bool*bool is AND
                opc = OP_OR if opc == OP_ADD else OP_AND
            return self.binary(opc, e.dtype, args[0], args[1])
        if op in ("floordiv", "mod"):
            d = args[1]
            xv = self.operand(args[0], e.dtype)
            code = _DT_CODE[e.dtype]
            if d & (d - 1) == 0:
                # floor semantics on two's complement: shift / mask
                if op == "floordiv":
                    opc, imm = OP_SHR, d.bit_length() - 1
                else:
                    opc, imm = OP_AND, d - 1
            else:
                opc = OP_FLOORDIV if op == "floordiv" else OP_MOD
                imm = _imm_bits(d, code)
            return self.emit((opc, code, xv, "imm", imm), opc, code,
                             (xv,), flags=FLAG_B_IMM, imm=imm)
        if op in ("lshift", "rshift"):
            opc = OP_SHL if op == "lshift" else OP_SHR
            code = _DT_CODE[e.dtype]
            xv = self.lower(args[0])
            return self.emit((opc, code, xv, "imm", args[1]), opc, code,
                             (xv,), flags=FLAG_B_IMM, imm=args[1])
        if op == "where":
            cv = self.lower(args[0])
            xv = self.operand(args[1], e.dtype)
            yv = self.operand(args[2], e.dtype)
            code = _DT_CODE[e.dtype]
            return self.emit((OP_WHERE, cv, xv, yv), OP_WHERE, code,
                             (cv, xv, yv))
        raise AssertionError(op)

    def lower_roots(self, roots: List[Expr]) -> List[int]:
        """Lower a section.  Its LOADs are emitted first, in slot order:
        the kernel issues them as one burst ahead of the arithmetic."""
        used = set()
        for e in roots:
            used |= e.columns()
        by_col = {}
        for e in roots:
            _collect_cols(e, by_col)
        for c in sorted(used):
            self.lower(by_col[c])
        return [self.lower(e) for e in roots]

    def allocate(self, roots: List[int]) -> Tuple[List[tuple], List[int],
                                                  int]:
        """Registers by liveness; roots stay live to the section's end.
        Returns (instrs, root registers, registers used)."""
        n = len(self.vals)
        last = list(range(n))
        for i, (_, _, srcs, *_r) in enumerate(self.vals):
            for s in srcs:
                last[s] = i
        for r in roots:
            last[r] = n
        free: List[int] = []
        nregs = 0
        reg = [0] * n
        instrs = []
        for i, (op, dt, srcs, c, flags, imm) in enumerate(self.vals):
            # operands are read before dst is written, so a source that
            # dies here may hand its register straight to the result
            for s in set(srcs):
                if last[s] == i:
                    free.append(reg[s])
            if free:
                free.sort(reverse=True)
                reg[i] = free.pop()
            else:
                reg[i] = nregs
                nregs += 1
            if last[i] == i:       # dead value (cannot happen for roots)
                free.append(reg[i])
            rs = [reg[s] for s in srcs] + [0, 0, 0]
            if op == OP_LOAD:
                a, b, cc = c, 0, 0
            elif op == OP_WHERE:
                a, b, cc = rs[0], rs[1], rs[2]
            else:
                a, b, cc = rs[0], rs[1], c
            instrs.append((op, dt, reg[i], a, b, cc, flags, imm))
        return instrs, [reg[r] for r in roots], nregs


def _collect_cols(e: Expr, out: dict) -> None:
    if e.op == "col":
        out[e.aux[0]] = e
    for a in e.args:
        if isinstance(a, Expr):
            _collect_cols(a, out)


_PROGRAMS: Dict[tuple, Program] = {}


def compile_program(outputs: Optional[Sequence[Expr]],
                    pred: Optional[Expr], in_schema: Schema) -> Program:
    """Lower typed Exprs over ``in_schema`` to a Program.  ``outputs``
    None means "every input column" (a pure filter).  A program over a
    limit, or one that must carry a BYTES/OBJECT column through a
    predicate, comes back with ``eligible`` False: not an error, the
    caller evaluates with torch instead."""
    if outputs is None:
        outputs = [col(i).bind(in_schema)
                   for i in range(in_schema.num_columns)]
    outputs = [e.bind(in_schema) for e in outputs]
    pred = pred.bind(in_schema) if pred is not None else None
    ckey = (tuple(e.key() for e in outputs),
            pred.key() if pred is not None else None)
    if ckey in _PROGRAMS:
        return _PROGRAMS[ckey]
    p = Program()
    p.out_dtypes = [e.dtype for e in outputs]

    def fail(reason):
        p.eligible, p.reason = False, reason
        _PROGRAMS[ckey] = p
        return p

    if pred is not None and pred.dtype != torch.bool:
        raise TypeError(f"predicate has dtype {pred.dtype}, not bool")
    computed = [e for e in outputs if pred is not None or e.op != "col"]
    for e in computed:
        if e.dtype not in _DT_CODE:
            return fail(f"a {e.dtype} column has to pass through a "
                        "predicate")
    used = set()
    for e in computed + ([pred] if pred is not None else []):
        used |= e.columns()
    p.inputs = sorted(used)
    p.in_dtypes = [in_schema.dtypes[i] for i in p.inputs]
    slot_of = {c: s for s, c in enumerate(p.inputs)}

    nregs = 0
    if pred is not None:
        lo = _Lower(slot_of)
        instrs, regs, nregs = lo.allocate(lo.lower_roots([pred]))
        p.instrs += instrs
        p.pred_reg = regs[0]
    p.n_pred = len(p.instrs)
    lo = _Lower(slot_of)
    instrs, regs, n2 = lo.allocate(lo.lower_roots(computed))
    p.instrs += instrs
    p.nregs = max(nregs, n2)
    it = iter(regs)
    p.outputs = [("reg", next(it)) if (pred is not None or e.op != "col")
                 else ("col", e.aux[0]) for e in outputs]

    if p.nregs > MAX_REGS:
        return fail(f"{p.nregs} registers > MAX_REGS")
    if len(p.instrs) > MAX_INSTRS:
        return fail(f"{len(p.instrs)} instructions > MAX_INSTRS")
    if len(p.inputs) > MAX_INPUTS:
        return fail(f"{len(p.inputs)} inputs > MAX_INPUTS")
    if len(computed) > MAX_OUTPUTS:
        return fail(f"{len(computed)} outputs > MAX_OUTPUTS")
    _PROGRAMS[ckey] = p
    return p


def run_program_host(program: Program, cols: Sequence):
    """Interpret the bytecode with torch ops, one instruction at a time,
    over a register list.  Returns (output columns before compaction,
    predicate mask or None).  It runs an over-limit program too: limits
    only decide native eligibility."""
    ins = [cols[i] for i in program.inputs]

    def lit(imm, code):
        import struct
        if code == _DT_F64:
            return struct.unpack("<d", struct.pack("<q", imm))[0]
        if code == _DT_F32:
            return struct.unpack("<f", struct.pack("<I", imm))[0]
        if code == _DT_BOOL:
            return bool(imm)
        return imm

    n = len(ins[0]) if ins else 0
    dev = ins[0].device if ins else "cpu"
    names = {OP_ADD: "add", OP_SUB: "sub", OP_MUL: "mul", OP_NEG: "neg",
             OP_ABS: "abs", OP_DIV: "truediv", OP_FLOORDIV: "floordiv",
             OP_MOD: "mod", OP_AND: "and", OP_OR: "or", OP_XOR: "xor",
             OP_NOT: "not", OP_SHL: "lshift", OP_SHR: "rshift",
             OP_EQ: "eq", OP_NE: "ne", OP_LT: "lt", OP_LE: "le",
             OP_GT: "gt", OP_GE: "ge", OP_MIN: "min", OP_MAX: "max"}

    def section(lo, hi):
        R: List = [None] * max(program.nregs, 1)
        for op, code, dst, a, b, c, flags, imm in program.instrs[lo:hi]:
            dt = DTYPES[code]
            if op == OP_CONST:
                v = torch.full((n,), lit(imm, code), dtype=dt, device=dev)
            elif op == OP_LOAD:
                v = ins[a]
                assert v.dtype == dt
            elif op == OP_CAST:
                assert R[a].dtype == DTYPES[c]
                v = R[a].to(dt)
            elif op == OP_WHERE:
                v = torch.where(R[a], R[b], R[c])
            else:
                x = R[a]
                assert x.dtype == dt, (op, x.dtype, dt)
                if flags & FLAG_B_IMM:
                    y = lit(imm, code)
                    if op in (OP_AND, OP_OR, OP_XOR, OP_MIN, OP_MAX) \
                            or OP_EQ <= op <= OP_GE:
                        # keep the operation at dt whatever Python type
                        # the immediate decoded to
                        y = torch.tensor(y, dtype=dt, device=dev)
                    args = [x, y]
                elif op in (OP_NEG, OP_ABS, OP_NOT):
                    args = [x]
                else:
                    assert R[b].dtype == dt
                    args = [x, R[b]]
                v = _apply(names[op], args, None)
                want = torch.bool if OP_EQ <= op <= OP_GE else dt
                assert v.dtype == want, (op, v.dtype, want)
            R[dst] = v
        return R

    keep = None
    if program.pred_reg >= 0:
        keep = section(0, program.n_pred)[program.pred_reg]
    R = section(program.n_pred, len(program.instrs))
    outs = [R[v] if kind == "reg" else cols[v]
            for kind, v in program.outputs]
    return outs, keep


# -- reader -----------------------------------------------------------------

class ExprSpec:
    """What one fused stage computes over its source frames: keep the
    rows where ``pred`` holds, emit ``outputs`` for them.  ``outputs``
    None is the identity (a pure filter, which also keeps the frame's
    prefix and combined_id, as Frame.mask does)."""

    def __init__(self, in_schema: Schema, outputs: Optional[List[Expr]],
                 pred: Optional[Expr], out_prefix: Optional[int]):
        self.in_schema = in_schema
        self.outputs = outputs
        self.pred = pred
        self.out_prefix = out_prefix
        self._program = None

    def then_map(self, exprs: List[Expr], prefix: int) -> "ExprSpec":
        if self.outputs is not None:
            exprs = [e.substitute(self.outputs) for e in exprs]
        return ExprSpec(self.in_schema, exprs, self.pred, prefix)

    def then_filter(self, pred: Expr) -> "ExprSpec":
        if self.outputs is not None:
            pred = pred.substitute(self.outputs)
        if self.pred is not None:
            pred = self.pred & pred
        return ExprSpec(self.in_schema, self.outputs, pred,
                        self.out_prefix)

    @property
    def program(self) -> Program:
        if self._program is None:
            self._program = compile_program(self.outputs, self.pred,
                                            self.in_schema)
        return self._program


class ExprReader(Reader):
    """Applies an ExprSpec to every frame of ``src``: one kernel launch
    per frame when the frame is on a GPU, the program is native-eligible
    and every column touched is a dense tensor of a supported dtype;
    ``Expr.eval`` then ``Frame.mask`` otherwise."""

    def __init__(self, src: Reader, spec: ExprSpec):
        self.src = src
        self.spec = spec
        self.started = False

    def close(self) -> None:
        self.src.close()

    def read(self) -> Optional[Frame]:
        self.started = True
        while True:
            f = self.src.read()
            if f is None:
                return None
            out = self._apply(f)
            if self.spec.pred is not None and len(out) == 0:
                continue
            return out

    def _frame(self, cols, f: Frame) -> Frame:
        if self.spec.outputs is None:
            return Frame(cols, f.prefix, combined_id=f.combined_id)
        return Frame(cols, self.spec.out_prefix)

    def _apply(self, f: Frame) -> Frame:
        from . import kernels
        spec = self.spec
        if f.device != "cpu" and spec.program.eligible \
                and kernels.expr_supported(spec.program, f):
            cols, _ = kernels.expr_apply(spec.program, f.columns)
            return self._frame(cols, f)
        keep = spec.pred.eval(f.columns) if spec.pred is not None else None
        if spec.outputs is None:
            return f.mask(keep)
        out = self._frame([e.eval(f.columns) for e in spec.outputs], f)
        return out.mask(keep) if keep is not None else out
