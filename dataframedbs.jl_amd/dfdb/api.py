"""Host-side mirror of DataFrameDBs.jl's lazy table algebra over the HIP engine.

Same names, argument meaning and error behaviour as the reference (paths under /root/reference):

    DFTable / open_table          src/tables/table.jl:9-56, src/tables/creators.jl:7-16
    DFView, selection, projection src/tables/view.jl:26-138
    DFColumn + broadcasting       src/tables/column.jl:30-126, src/tables/columnbroadcast.jl:1-72
    SelectionQueue composition    src/tables/selection.jl:4-60
    Projection                    src/tables/projection.jl:1-97
    materialize / nrow / size     src/tables/materialization.jl:27-56, src/tables/view.jl:192-232

Julia idioms map to Python as follows (rows stay 1-BASED, ranges inclusive, like the reference):

    t[:, :]                      t[ALL, ALL]           (or t[:, :])
    t[5:20, [:a, :c]]            t[jr(5, 20), ["a", "c"]]
    t[1:2:end, :a]               t[jr(1, 2, END), "a"]
    :a => f  /  (:a,:b) => f     ("a", f)  /  (("a", "b"), f)
    (e = :a, k = (:a,:c) => f)   {"e": "a", "k": (("a", "c"), f)}
    t.a .> 5  /  a .& b          t.a > 5   /  a & b          (DFColumn operators build the same trees)
    startswith.(t.b, "1")        startswith(t.b, "1")
    dest .= t.a .* t.c           (t.a * t.c).copyto(dest)

Everything data-parallel runs in libdfdb_hip.so; this module only builds queries.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native as N
from . import ir


# ---------------------------------------------------------------- selectors
class _All:
    def __repr__(self): return ":"


ALL = _All()


class _End:
    """Julia's `end` inside an index expression: resolved with lastindex(v, dim) (view.jl:227-232)."""

    def __init__(self, offset: int = 0): self.offset = offset
    def __add__(self, k: int): return _End(self.offset + int(k))
    def __sub__(self, k: int): return _End(self.offset - int(k))
    def resolve(self, n: int) -> int: return n + self.offset
    def __repr__(self): return "end" + (f"{self.offset:+d}" if self.offset else "")


END = _End()


class JRange:
    """Julia `a:b` / `a:s:b`: 1-based, inclusive."""

    def __init__(self, start, step, stop):
        self.start, self.step, self.stop = start, step, stop

    def resolved(self, n: int) -> "JRange":
        f = lambda x: x.resolve(n) if isinstance(x, _End) else int(x)
        return JRange(f(self.start), int(self.step), f(self.stop))

    def has_end(self) -> bool:
        return isinstance(self.start, _End) or isinstance(self.stop, _End)

    def __len__(self):
        a, s, b = int(self.start), int(self.step), int(self.stop)
        return max(0, (b - a) // s + 1) if s > 0 else max(0, (a - b) // (-s) + 1)

    def __iter__(self):
        a, s = int(self.start), int(self.step)
        return (a + k * s for k in range(len(self)))

    def __eq__(self, o): return isinstance(o, JRange) and list(self) == list(o)
    def __hash__(self): return hash((self.start, self.step, self.stop))
    def __repr__(self): return f"{self.start}:{self.step}:{self.stop}" if self.step != 1 else f"{self.start}:{self.stop}"


def jr(a, b, c=None) -> JRange:
    """jr(a, b) == a:b ; jr(a, s, b) == a:s:b"""
    return JRange(a, 1, b) if c is None else JRange(a, b, c)


def _is_colon(x) -> bool:
    return x is ALL or x is Ellipsis or (isinstance(x, slice) and x == slice(None))


# ---------------------------------------------------------------- SelectionQueue (selection.jl:4-60)
class SelectionQueue:
    """Immutable tuple of stages: JRange | int | list[int] | ir.Expr (Bool)."""

    def __init__(self, queue: Tuple = ()):
        self.queue = tuple(queue)

    def __len__(self): return len(self.queue)
    def isempty(self): return not self.queue

    @staticmethod
    def _index(old, elem):
        """old[elem] with Julia bounds checking (range∘range collapse, selection.jl:40)."""
        def at(k: int):
            if isinstance(old, int):
                if k != 1:
                    raise IndexError("BoundsError: indexing a scalar selection")
                return old
            n = len(old)
            if k < 1 or k > n:
                raise IndexError(f"BoundsError: attempt to access {n}-element selection at index [{k}]")
            return (old.start + (k - 1) * old.step) if isinstance(old, JRange) else old[k - 1]
        if isinstance(elem, int):
            return at(elem)
        if isinstance(old, int):
            raise IndexError("BoundsError: indexing a scalar selection")
        if isinstance(old, JRange) and isinstance(elem, JRange):
            if len(elem) == 0:
                return JRange(old.start, old.step * elem.step, old.start - old.step * elem.step)
            return JRange(at(elem.start), old.step * elem.step, at(elem.start + (len(elem) - 1) * elem.step))
        return [at(k) for k in elem]

    def add(self, elem) -> "SelectionQueue":
        if _is_colon(elem):
            return self                                                    # add(q, ::Colon) = q (:37)
        if isinstance(elem, ir.Expr):
            if not self.queue or not isinstance(self.queue[-1], ir.Expr):
                return SelectionQueue(self.queue + (elem,))
            return SelectionQueue(self.queue[:-1] + (self.queue[-1] & elem,))   # fuse with & (:44-47)
        if not isinstance(elem, (JRange, int, list)):
            raise TypeError(f"unsupported selection element {elem!r}")
        if self.queue and not isinstance(self.queue[-1], ir.Expr):
            return SelectionQueue(self.queue[:-1] + (self._index(self.queue[-1], elem),))
        return SelectionQueue(self.queue + (elem,))

    def same(self, o: "SelectionQueue") -> bool:
        if len(self.queue) != len(o.queue):
            return False
        for a, b in zip(self.queue, o.queue):
            if isinstance(a, ir.Expr) != isinstance(b, ir.Expr):
                return False
            if isinstance(a, ir.Expr):
                if not _expr_equal(a, b):
                    return False
            elif type(a) is not type(b) or (list(a) if not isinstance(a, int) else a) != (list(b) if not isinstance(b, int) else b):
                return False
        return True

    def __repr__(self):
        return "Selection: " + " |> ".join(map(repr, self.queue))


def _expr_equal(a: ir.Expr, b: ir.Expr) -> bool:
    """View equality compares the stored objects (view.jl:34-38, quirk Q12): traces of two distinct
    closures differ even if structurally equal; the same function object compares equal."""
    fa, fb = getattr(a, "_origin", None), getattr(b, "_origin", None)
    if fa is not None or fb is not None:
        return fa is fb and a.same(b)
    return a.same(b)


class _TracedExpr(ir.Expr):
    __slots__ = ("_origin",)


def _trace(fn: Callable, leaves: Sequence[ir.Expr]) -> ir.Expr:
    e = ir.trace(fn, leaves)
    t = _TracedExpr(e.op, e.args, e.payload)
    t._origin = fn
    return t


# ---------------------------------------------------------------- Projection (projection.jl:1-97)
class Projection:
    """Ordered output-name -> ir.Expr (a plain column is `ir.col(k)`)."""

    def __init__(self, cols: Optional[Dict[str, ir.Expr]] = None):
        self.cols: Dict[str, ir.Expr] = dict(cols or {})

    def keys(self) -> List[str]: return list(self.cols.keys())
    def __len__(self): return len(self.cols)

    def add(self, el: Dict[str, ir.Expr]) -> "Projection":
        for k in el:
            if k in self.cols:
                raise ValueError(f"ArgumentError: Duplicated column {k}")      # projection.jl:25-28
        d = dict(self.cols)
        d.update(el)
        return Projection(d)

    def select_positions(self, idx: Sequence[int]) -> "Projection":            # getindex by Integer positions (:43-54)
        ks = self.keys()
        out = {}
        for i in idx:
            if i < 1 or i > len(ks):
                raise IndexError(f"BoundsError: projection has {len(ks)} columns, index [{i}]")
            out[ks[i - 1]] = self.cols[ks[i - 1]]
        return Projection(out)

    def select_names(self, names: Sequence[str]) -> "Projection":              # _get_indexes keeps PROJECTION order (:55-75, Q13)
        return Projection({k: v for k, v in self.cols.items() if k in names})

    def same(self, o: "Projection") -> bool:
        return self.keys() == o.keys() and all(_expr_equal(self.cols[k], o.cols[k]) for k in self.cols)

    def __repr__(self):
        return "Projection: " + "; ".join(f"{k}=>{v!r}" for k, v in self.cols.items())


# ---------------------------------------------------------------- engine handles
class Context:
    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self._h = C.c_void_p()
        N.check(N.load().dfdb_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self._h)))
        self.device = device

    def synchronize(self): N.check(N.load().dfdb_ctx_synchronize(self._h))

    def device_info(self) -> dict:
        d = N.DeviceInfo()
        N.check(N.load().dfdb_ctx_device_info(self._h, C.byref(d)))
        return dict(name=d.name.decode(), compute_units=d.compute_units, wavefront_size=d.wavefront_size, hbm_bytes=d.hbm_bytes,
                    peak_hbm_gbps=d.peak_hbm_gbps)

    def set_option(self, key: str, value: int): N.check(N.load().dfdb_ctx_set_option(self._h, key.encode(), value))

    def timer_start(self): N.check(N.load().dfdb_ctx_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = C.c_double()
        N.check(N.load().dfdb_ctx_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def profile(self, on: bool): N.check(N.load().dfdb_ctx_profile_enable(self._h, 1 if on else 0))

    def profile_get(self, kernel: str) -> Tuple[int, float]:
        n, ms = C.c_int64(), C.c_double()
        N.check(N.load().dfdb_ctx_profile_get(self._h, kernel.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def close(self):
        if self._h:
            N.load().dfdb_ctx_destroy(self._h)
            self._h = C.c_void_p()


_default_ctx: Dict[int, Context] = {}


def default_context(device: int = 0) -> Context:
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


class ColumnMeta:
    def __init__(self, id: int, name: str, dtype: int, logical: str = ""):
        self.id, self.name, self.dtype, self.logical = id, name, dtype, logical

    @property
    def type(self) -> str:
        if not self.logical:
            return ir.dtype_name(self.dtype)
        return f"Missing({self.logical})" if self.dtype & ir.NULLABLE else self.logical     # Date / DateTime / Time / Char
    def __eq__(self, o): return isinstance(o, ColumnMeta) and (self.id, self.name, self.dtype, self.logical) == (o.id, o.name, o.dtype, o.logical)
    def __repr__(self): return f"ColumnMeta({self.id}, :{self.name}, {self.type})"


class DFTable:
    """A table whose columns are decoded and resident in HBM (struct DFTable: table.jl:9-15)."""

    def __init__(self, handle, ctx: Context, path: str = ""):
        object.__setattr__(self, "_h", handle)
        object.__setattr__(self, "ctx", ctx)
        object.__setattr__(self, "path", path)
        object.__setattr__(self, "is_opened", True)

    # -- construction
    @classmethod
    def new(cls, block_size: int = 65536, ctx: Optional[Context] = None) -> "DFTable":
        ctx = ctx or default_context()
        h = C.c_void_p()
        N.check(N.load().dfdb_table_new(ctx._h, C.c_int64(block_size), C.byref(h)))
        return cls(h, ctx)

    @classmethod
    def from_columns(cls, columns: Dict[str, Any], block_size: int = 65536, ctx: Optional[Context] = None) -> "DFTable":
        """In-memory table from host arrays (numpy / list[str|None] / masked arrays): the data path of
        create_table(path; from = df) (creators.jl:81-89) without the files."""
        t = cls.new(block_size, ctx)
        for name, v in columns.items():
            t.add_column(name, v)
        return t

    def add_column(self, name: str, values, dtype: Optional[int] = None, logical: Optional[str] = None):
        """values: numpy array (datetime64 / timedelta64 become Date / DateTime / Time columns), masked array, or a list of str / None.
        logical="Char" with 1-character strings makes a Char column.  A lazy DFColumn (or one-column DFView) is add_column!(table, name, lazy_col):
        add_column_from."""
        if isinstance(values, (DFColumn, DFView)):
            return self.add_column_from(name, values)
        L = N.load()
        if logical == "Char":
            values = np.array([ir.julia_char(c) for c in values], np.uint32)
        elif isinstance(values, np.ndarray) and values.dtype.kind in "Mm":
            fill = None
            if isinstance(values, np.ma.MaskedArray):
                fill = np.ma.getmaskarray(values); values = values.filled(values.dtype.type(0))
            if values.dtype.kind == "m":
                ints, logical = values.astype("timedelta64[ns]").astype(np.int64), "Time"
            elif np.datetime_data(values.dtype)[0] in ("D", "W", "M", "Y"):
                ints, logical = values.astype("datetime64[D]").astype(np.int64) + ir.RATA_DIE_DAYS, "Date"
            else:
                ints, logical = values.astype("datetime64[ms]").astype(np.int64) + ir.RATA_DIE_MS, "DateTime"
            values = np.ma.masked_array(ints, mask=fill) if fill is not None else ints
        if logical:
            self.add_column(name, values, dtype)
            N.check(L.dfdb_table_set_logical_type(self._h, self.ordinal(name), logical.encode()))
            return
        if isinstance(values, (list, tuple)) and (len(values) == 0 or isinstance(values[0], (str, bytes, type(None)))) and not isinstance(values, np.ndarray):
            enc = [None if v is None else (v.encode() if isinstance(v, str) else bytes(v)) for v in values]
            sizes = np.array([-1 if e is None else len(e) for e in enc], np.int32)
            data = np.frombuffer(b"".join(e for e in enc if e), np.uint8).copy()
            dt = ir.STRING | (ir.NULLABLE if any(e is None for e in enc) or (dtype or 0) & ir.NULLABLE else 0)
            N.check(L.dfdb_table_add_column(self._h, name.encode(), dt, len(sizes), sizes.ctypes.data, data.ctypes.data if len(data) else None,
                                            len(data), None))
            return
        missing = None
        if isinstance(values, np.ma.MaskedArray):
            missing = np.ascontiguousarray(np.ma.getmaskarray(values), np.uint8)
            values = values.filled(0)
        arr = np.ascontiguousarray(values)
        if dtype is None:
            dtype = ir.dtype_of_numpy(arr.dtype)
        arr = np.ascontiguousarray(arr.astype(ir.numpy_of_dtype(dtype), copy=False))
        if missing is not None:
            dtype |= ir.NULLABLE
        N.check(L.dfdb_table_add_column(self._h, name.encode(), dtype, len(arr), arr.ctypes.data if len(arr) else None, None, 0,
                                        missing.ctypes.data if missing is not None else None))

    def add_generated(self, name: str, generator: int, seed: int, nrows: int, row_first: int = 0):
        N.check(N.load().dfdb_table_add_generated(self._h, name.encode(), generator, C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), row_first, nrows))

    def load(self, columns: Optional[Sequence[str]] = None, block_first: int = 0, block_last: int = -1) -> dict:
        """Decode blocks [block_first, block_last) of the listed columns into HBM (read_block! for every block)."""
        st = N.SizeStats()
        if columns is None:
            N.check(N.load().dfdb_table_load(self._h, None, 0, block_first, block_last, C.byref(st)))
        else:
            ords = (C.c_int32 * len(columns))(*[self.ordinal(c) for c in columns])
            N.check(N.load().dfdb_table_load(self._h, ords, len(columns), block_first, block_last, C.byref(st)))
        return dict(rows=st.rows, compressed=st.compressed, uncompressed=st.uncompressed)

    def load_image(self, column: str, image: bytes, block_first: int = 0, block_last: int = -1) -> dict:
        st = N.SizeStats()
        N.check(N.load().dfdb_table_load_image(self._h, self.ordinal(column), image, len(image), block_first, block_last, C.byref(st)))
        return dict(rows=st.rows, compressed=st.compressed, uncompressed=st.uncompressed)

    def decode_resident(self, column: str):
        """K7 over the LZ4 blocks the column kept in HBM (ctx option keep_compressed at load time), asynchronously"""
        N.check(N.load().dfdb_table_decode_resident(self._h, self.ordinal(column)))

    def decode_status(self, column: str) -> int:
        """blocks of the column's last resident decode that did not end with their stored size (0 = fine); waits for the stream"""
        bad = C.c_int64()
        N.check(N.load().dfdb_table_decode_status(self._h, self.ordinal(column), C.byref(bad)))
        return bad.value

    def compress_column(self, column: str, mode: int = 2) -> dict:
        """a resident plain fixed-width column -> compressed-resident (mode 1) or compressed-only (mode 2) in HBM, encoded on the device: dfdb_table_compress_column"""
        st = N.SizeStats()
        N.check(N.load().dfdb_table_compress_column(self._h, self.ordinal(column), mode, C.byref(st)))
        return dict(rows=st.rows, compressed=st.compressed, uncompressed=st.uncompressed)

    def resident_bytes(self, column=None) -> dict:
        """HBM bytes held right now by one column (or the whole table): {"decoded": ..., "compressed": ...} — dfdb_table_resident_bytes"""
        d, k = C.c_int64(), C.c_int64()
        N.check(N.load().dfdb_table_resident_bytes(self._h, -1 if column is None else self.ordinal(column), C.byref(d), C.byref(k)))
        return {"decoded": d.value, "compressed": k.value}

    def read_probe(self, column: str, repeats: int = 5):
        """(best_ms, avg_ms) of K1's read stream alone over a resident 8-byte column: dfdb_table_read_probe"""
        best, avg = C.c_double(), C.c_double()
        N.check(N.load().dfdb_table_read_probe(self._h, self.ordinal(column), repeats, C.byref(best), C.byref(avg)))
        return best.value, avg.value

    def build_dictionary(self, column: str, max_entries: int = 4096) -> int:
        """K9: 16-bit codes + the distinct strings of a resident String column (kept beside its flat form); returns the number of distinct
        strings, 0 when none was built (more than max_entries, nullable, a string over 4 KB).  Results of every query stay the same."""
        n = C.c_int64()
        N.check(N.load().dfdb_table_build_dictionary(self._h, self.ordinal(column), max_entries, C.byref(n)))
        return n.value

    def set_row_base(self, row_base: int): N.check(N.load().dfdb_table_set_row_base(self._h, row_base))

    def add_column_from(self, name: str, col) -> None:
        """add_column!(table, name, lazy_col) (table.jl:96-124): a DFColumn (or one-column DFView), plain or computed,
        filtered or not, becomes a new resident column of this table without leaving the device."""
        v = col.view if isinstance(col, DFColumn) else col
        if not isinstance(v, DFView) or len(v.projection) != 1:
            raise ValueError("ArgumentError: add_column_from needs a DFColumn or a one-column DFView")
        q = v._query()
        N.check(N.load().dfdb_table_add_from_query(self._h, name.encode(), q._h, 0))

    def save(self, path: str) -> dict:
        """create_table(path; from=table) (creators.jl:18-60): every resident column to `<path>/<id>.bin` in the reference's
        block format (bodies packed + LZ4-compressed on the device) and `<path>/meta.bin`.  Returns the SizeStats."""
        st = N.SizeStats()
        N.check(N.load().dfdb_table_save(self._h, os.fsencode(path), C.byref(st)))
        return {"rows": st.rows, "compressed": st.compressed, "uncompressed": st.uncompressed}

    def save_column(self, name: str, file: str) -> dict:
        st = N.SizeStats()
        N.check(N.load().dfdb_table_save_column(self._h, self.ordinal(name), os.fsencode(file), C.byref(st)))
        return {"rows": st.rows, "compressed": st.compressed, "uncompressed": st.uncompressed}

    def close(self):
        if self._h:
            N.load().dfdb_table_close(self._h)
            object.__setattr__(self, "_h", C.c_void_p())
            object.__setattr__(self, "is_opened", False)

    # -- metadata (table.jl:23-56)
    @property
    def ncols(self) -> int:
        n = C.c_int32()
        N.check(N.load().dfdb_table_ncols(self._h, C.byref(n)))
        return n.value

    def columns_meta(self) -> List[ColumnMeta]:
        out = []
        for i in range(self.ncols):
            ci = N.ColInfo()
            N.check(N.load().dfdb_table_colinfo(self._h, i, C.byref(ci)))
            out.append(ColumnMeta(ci.id, ci.name.decode(), ci.dtype, ci.logical.decode()))
        return out

    def names(self) -> List[str]: return [m.name for m in self.columns_meta()]

    def resident(self, ordinal: int) -> bool:
        ci = N.ColInfo()
        N.check(N.load().dfdb_table_colinfo(self._h, ordinal, C.byref(ci)))
        return bool(ci.resident)

    def ordinal(self, name: str) -> int:
        o = C.c_int32()
        N.check(N.load().dfdb_table_find_column(self._h, name.encode(), C.byref(o)))
        return o.value

    def getmeta(self, name: str) -> ColumnMeta: return self.columns_meta()[self.ordinal(name)]

    @property
    def blocksize(self) -> int:
        b = C.c_int64()
        N.check(N.load().dfdb_table_block_size(self._h, C.byref(b)))
        return b.value

    def expr_dtype(self, e: ir.Expr) -> int:
        dt = C.c_int32()
        b = e.to_ir()
        N.check(N.load().dfdb_expr_result_type(self._h, b, len(b), C.byref(dt)))
        return dt.value

    def expr_logical(self, e: ir.Expr) -> str:
        """the bits type the result dtype stands for: "DateTime" for datetime19(s), a plain column's own, "" otherwise (dfdb_expr_result_logical)"""
        buf = C.create_string_buffer(32)
        b = e.to_ir()
        N.check(N.load().dfdb_expr_result_logical(self._h, b, len(b), buf, len(buf)))
        return buf.value.decode()

    def __eq__(self, o):     # table.jl:18-21: path + column metas only (quirk Q12)
        return isinstance(o, DFTable) and (self is o or (self.path != "" and self.path == o.path and self.columns_meta() == o.columns_meta()))

    def __hash__(self): return id(self)

    # -- DFTable indexing proxies to the full view (view.jl:138,174-177)
    def view(self) -> "DFView": return DFView(self)
    def __getitem__(self, key): return DFView(self)[key]

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        try:
            return DFView(self)[ALL, name]
        except (KeyError, ValueError):
            raise AttributeError(name) from None

    def __repr__(self): return f"DFTable({self.path!r}, {self.columns_meta()})"


def open_table(path: str, device: int = 0, ctx: Optional[Context] = None, load: bool = True, block_first: int = 0,
               block_last: int = -1) -> DFTable:
    """open_table(path) (creators.jl:7-16); with load=True all blocks in the range are decoded into HBM."""
    ctx = ctx or default_context(device)
    h = C.c_void_p()
    N.check(N.load().dfdb_table_open(ctx._h, path.encode(), C.byref(h)))
    t = DFTable(h, ctx, path)
    if load:
        t.load(None, block_first, block_last)
    return t


# ---------------------------------------------------------------- DFView (view.jl:26-232)
Selector = Any
Projector = Any


class DFView:
    def __init__(self, table: DFTable, projection: Optional[Projection] = None, selection: Optional[SelectionQueue] = None):
        self.table = table
        if projection is None:   # full_table_projection (view.jl:43-48)
            projection = Projection({m.name: ir.col(i) for i, m in enumerate(table.columns_meta())})
        self.projection = projection
        self.selection = selection or SelectionQueue()
        self._q = None

    # -- selection(v, el) (view.jl:60-72, column.jl:72-75)
    def _selection(self, el) -> "DFView":
        if _is_colon(el):
            return self
        if isinstance(el, DFColumn):
            if el.eltype != ir.BOOL:
                raise ValueError("ArgumentError: Function for selection must have Bool result type")
            if not self.selection.same(el.view.selection):
                raise ValueError("ArgumentError: col must have same selection as view")
            return DFView(self.table, self.projection, self.selection.add(el.expr))
        if isinstance(el, tuple) and len(el) == 2 and callable(el[1]):      # cols => f
            cols = [el[0]] if isinstance(el[0], str) else list(el[0])
            for c in cols:
                if c not in self.projection.cols:
                    raise ValueError(f"ArgumentError: view don't have column :{c}")
            args = list(self.projection.select_names(cols).cols.values())     # projection order (quirk Q13)
            e = _trace(el[1], args)
            if self.table.expr_dtype(e) != ir.BOOL:
                raise ValueError("ArgumentError: Function for selection must have Bool result type")   # selection.jl:52-55
            return DFView(self.table, self.projection, self.selection.add(e))
        if isinstance(el, ir.Expr):
            if self.table.expr_dtype(el) != ir.BOOL:
                raise ValueError("ArgumentError: Function for selection must have Bool result type")
            return DFView(self.table, self.projection, self.selection.add(el))
        if isinstance(el, (bool, np.bool_)):
            raise TypeError("Bool masks enter only as lazy DFColumn{Bool} (quirk Q4)")
        if isinstance(el, (int, np.integer)):
            return DFView(self.table, self.projection, self.selection.add(int(el)))
        if isinstance(el, _End):
            return DFView(self.table, self.projection, self.selection.add(el.resolve(nrow(self))))
        if isinstance(el, JRange):
            r = el.resolved(nrow(self)) if el.has_end() else el.resolved(0)
            if r.step == 0:
                raise ValueError("ArgumentError: step cannot be zero")
            return DFView(self.table, self.projection, self.selection.add(r))
        if isinstance(el, (list, np.ndarray)):
            arr = np.asarray(el)
            if arr.dtype == bool:
                raise TypeError("Bool masks enter only as lazy DFColumn{Bool} (quirk Q4)")
            return DFView(self.table, self.projection, self.selection.add(arr.astype(np.int64).tolist()))
        raise TypeError(f"unsupported selector {el!r}; use jr(a, b) for ranges (1-based, inclusive)")

    # -- projection(v, p) (view.jl:75-109)
    def _proj_elem(self, elem) -> ir.Expr:
        if isinstance(elem, str):
            if elem not in self.projection.cols:
                raise ValueError(f"ArgumentError: view don't have column :{elem}")
            return self.projection.cols[elem]
        if isinstance(elem, tuple) and len(elem) == 2 and callable(elem[1]):
            cols = [elem[0]] if isinstance(elem[0], str) else list(elem[0])
            return _trace(elem[1], [self._proj_elem(c) for c in cols])          # tuple order (quirk Q13)
        if isinstance(elem, DFColumn):
            return elem.expr
        raise TypeError(f"unsupported projection element {elem!r}")

    def _projection(self, p) -> "DFView":
        if _is_colon(p):
            return self
        if isinstance(p, dict):
            return DFView(self.table, Projection({k: self._proj_elem(v) for k, v in p.items()}), self.selection)
        if isinstance(p, JRange):
            return DFView(self.table, self.projection.select_positions(list(p.resolved(len(self.projection)))), self.selection)
        if isinstance(p, (list, tuple)):
            if all(isinstance(x, str) for x in p):
                if len(set(p)) != len(p):
                    raise ValueError(f"ArgumentError: Duplicated column")
                return self._projection({x: x for x in p})
            if all(isinstance(x, (int, np.integer)) for x in p):
                return DFView(self.table, self.projection.select_positions([int(x) for x in p]), self.selection)
            if all(isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], str) for x in p):   # Vector{Pair}: [:a=>:a, :c=>:c=>f]
                return self._projection({k: v for k, v in p})
        raise TypeError(f"unsupported projector {p!r}")

    def __getitem__(self, key):
        if not isinstance(key, tuple) or len(key) != 2:
            raise TypeError("index a view as v[selector, projector]")
        s, p = key
        # getindex(v, s, p::Union{Number,Symbol}) -> DFColumn (view.jl:123-128)
        single = isinstance(p, (str, int, np.integer)) or (isinstance(p, _End)) or (isinstance(p, tuple) and len(p) == 2 and callable(p[1]))
        if single:
            if isinstance(p, _End):
                p = p.resolve(len(self.projection))
            base = self._selection(s)
            pv = base._projection({"a": p}) if isinstance(p, tuple) else base._projection([p])
            col = DFColumn(pv)
            if isinstance(s, (int, np.integer)) and not isinstance(s, bool):
                return col._scalar()                                          # view.jl:125
            return col
        if isinstance(s, (int, np.integer)) and not isinstance(s, bool):       # getindex(v, s::Number, p::Any) -> first row (view.jl:130-135)
            v = self._selection([int(s)])._projection(p)
            df = materialize(v)
            if len(df) == 0:
                raise IndexError(f"BoundsError: attempt to access view at index [{s}]")
            return {k: df[k].iloc[0] for k in df.columns}
        if _is_colon(s) and _is_colon(p):
            return self
        return self._selection(s)._projection(p)

    def __getattr__(self, name):   # getproperty(v, name) = v[:, name] (view.jl:167-170)
        if name.startswith("_") or name in ("table", "projection", "selection"):
            raise AttributeError(name)
        try:
            return self[ALL, name]
        except ValueError:
            raise AttributeError(name) from None

    def names(self) -> List[str]: return self.projection.keys()

    def __eq__(self, o):          # view.jl:34-38
        return isinstance(o, DFView) and self.table == o.table and self.projection.same(o.projection) and self.selection.same(o.selection)

    def __ne__(self, o): return not self.__eq__(o)
    def __hash__(self): return id(self)

    def required_columns(self) -> List[str]:   # view.jl:183-190
        ords: List[int] = []
        for e in self.projection.cols.values():
            for c in e.columns():
                if c not in ords:
                    ords.append(c)
        for st in self.selection.queue:
            if isinstance(st, ir.Expr):
                for c in st.columns():
                    if c not in ords:
                        ords.append(c)
        nm = self.table.names()
        return [nm[c] for c in ords]

    # -- engine query (built once per immutable view)
    def _query(self):
        if self._q is None:
            self._q = _Query(self)
        return self._q

    def __repr__(self):
        return f"View of table {self.table.path}\n{self.projection}\n{self.selection}"


def issameselection(a: DFView, b: DFView) -> bool:   # view.jl:180-181
    return a.table == b.table and a.selection.same(b.selection)


def selection(v: Union[DFView, DFTable], el) -> DFView:
    return (v if isinstance(v, DFView) else DFView(v))._selection(el)


def projection(v: Union[DFView, DFTable], p) -> DFView:
    return (v if isinstance(v, DFView) else DFView(v))._projection(p)


def selproj(v: DFView, select, project) -> DFView:   # view.jl:112-118
    return v._selection(select)._projection(project)


# ---------------------------------------------------------------- engine query wrapper
class _Query:
    def __init__(self, v: DFView):
        L = N.load()
        self.view = v
        self._h = C.c_void_p()
        N.check(L.dfdb_query_new(v.table._h, C.byref(self._h)))
        try:
            for st in v.selection.queue:
                if isinstance(st, ir.Expr):
                    b = st.to_ir()
                    N.check(L.dfdb_query_add_predicate(self._h, b, len(b)))
                elif isinstance(st, JRange):
                    N.check(L.dfdb_query_add_range(self._h, int(st.start), int(st.step), int(st.stop)))
                elif isinstance(st, int):
                    N.check(L.dfdb_query_add_integer(self._h, st))
                else:
                    a = np.ascontiguousarray(st, np.int64)
                    N.check(L.dfdb_query_add_indices(self._h, a.ctypes.data if len(a) else None, len(a)))
            items = [(k, e.to_ir()) for k, e in v.projection.cols.items()]
            n = len(items)
            names = (C.c_char_p * max(n, 1))(*[k.encode() for k, _ in items])
            bufs = [C.create_string_buffer(b, len(b)) for _, b in items]
            irs = (C.c_void_p * max(n, 1))(*[C.cast(b, C.c_void_p) for b in bufs])
            lens = (C.c_size_t * max(n, 1))(*[len(b) for _, b in items])
            N.check(L.dfdb_query_set_projection(self._h, n, names, irs, lens))
        except Exception:
            L.dfdb_query_free(self._h)
            self._h = C.c_void_p()
            raise

    def __del__(self):
        try:
            import sys
            if self._h and not sys.is_finalizing():    # never call into HIP while the interpreter tears down
                N.load().dfdb_query_free(self._h)
        except Exception:
            pass

    def execute(self): N.check(N.load().dfdb_query_execute(self._h))

    def reset(self): N.check(N.load().dfdb_query_reset(self._h))

    def count(self) -> int:
        n = C.c_int64()
        N.check(N.load().dfdb_count(self._h, C.byref(n)))
        return n.value

    def count_device(self, dev_ptr: int):
        N.check(N.load().dfdb_count_to(self._h, C.c_void_p(dev_ptr), N.MEM_DEVICE))

    def coltype(self, i: int) -> int:
        dt = C.c_int32()
        N.check(N.load().dfdb_query_coltype(self._h, i, C.byref(dt)))
        return dt.value

    def indices(self) -> np.ndarray:
        n = self.count()
        out = np.empty(n, np.int64)
        got = C.c_int64()
        N.check(N.load().dfdb_select_indices(self._h, out.ctypes.data if n else None, n, N.MEM_HOST, C.byref(got)))
        return out

    def indices_device(self, dev_ptr: int, cap: int, want_count: bool = False) -> Optional[int]:
        got = C.c_int64()
        N.check(N.load().dfdb_select_indices(self._h, C.c_void_p(dev_ptr), cap, N.MEM_DEVICE, C.byref(got) if want_count else None))
        return got.value if want_count else None

    def bitmap(self) -> np.ndarray:
        nrows = C.c_int64()
        N.check(N.load().dfdb_table_nrows(self.view.table._h, C.byref(nrows)))
        out = np.zeros((nrows.value + 63) // 64, np.uint64)
        if len(out):
            N.check(N.load().dfdb_select_bitmap(self._h, out.ctypes.data, N.MEM_HOST))
        return out

    def hint_materialize(self, on: bool = True):
        N.check(N.load().dfdb_query_hint_materialize(self._h, 1 if on else 0))

    def _columns_out(self, n: int, fill, string_bytes=None) -> List[Any]:
        """n rows of every projection column through host outputs that fill(outs, ncols) has the library write: a String column as (int32 sizes, bytes), its
        buffer sized by string_bytes(i) (None: it gets no buffer — the library refuses it by name), a nullable fixed-width column masked"""
        ncols = len(self.view.projection)
        outs = (N.OutCol * max(ncols, 1))()
        keep = []
        for i in range(ncols):
            dt = self.coltype(i)
            o = outs[i]
            o.memkind = N.MEM_HOST
            if (dt & ir.DTYPE_MASK) == ir.STRING:
                if string_bytes is None:
                    keep.append((dt, None, None, None))
                    continue
                nb = string_bytes(i)
                sizes = np.empty(max(n, 1), np.int32)
                data = np.empty(max(nb, 1), np.uint8)
                keep.append((dt, sizes, data, None))
                o.data, o.bytes, o.bytes_cap = sizes.ctypes.data, data.ctypes.data, nb
            else:
                arr = np.empty(max(n, 1), ir.numpy_of_dtype(dt))
                miss = np.zeros(max(n, 1), np.uint8) if dt & ir.NULLABLE else None
                keep.append((dt, arr, None, miss))
                o.data = arr.ctypes.data
                if miss is not None:
                    o.missing = miss.ctypes.data
        fill(outs, ncols)
        res = []
        for i, (dt, a, b, m) in enumerate(keep):
            if (dt & ir.DTYPE_MASK) == ir.STRING:
                res.append((a[:n].copy(), b[:outs[i].nbytes].copy()))
            elif m is not None:
                res.append(np.ma.masked_array(a[:n].copy(), mask=m[:n].astype(bool)))
            else:
                res.append(a[:n].copy())
        return res

    def materialize(self) -> List[Any]:
        L = N.load()
        self.hint_materialize(True)       # count() below is the scan: let it keep projected predicate columns

        def string_bytes(i):
            nb = C.c_int64()
            N.check(L.dfdb_result_string_bytes(self._h, i, C.byref(nb)))
            return nb.value

        return self._columns_out(self.count(), lambda outs, ncols: N.check(L.dfdb_materialize(self._h, outs, ncols)) if ncols else None, string_bytes)

    def hint_aggregate(self, op: int, col: int = 0):
        N.check(N.load().dfdb_query_hint_aggregate(self._h, op, col))

    def aggregate(self, op: int, col: int = 0):
        oi, of = C.c_int64(), C.c_double()
        if op in (N.AGG_SUM, N.AGG_MIN, N.AGG_MAX):
            self.hint_aggregate(op, col)      # a first execution below lets the scan reduce the column while it holds it
        N.check(N.load().dfdb_aggregate(self._h, op, col, C.byref(oi), C.byref(of)))
        dt = self.coltype(col) & ir.DTYPE_MASK if op != N.AGG_COUNT else ir.I64
        if dt in (ir.F32, ir.F64):
            return of.value
        # Base.sum widens unsigned element types to UInt64 (Base.add_sum), minimum / maximum keep them: the 64 bits are an unsigned number
        return oi.value & 0xFFFFFFFFFFFFFFFF if dt in (ir.U8, ir.U16, ir.U32, ir.U64) else oi.value

    def order_statistics(self, ranks, col: int = 0):
        """dfdb_order_statistics: the values at the 1-based `ranks` (any number: 16 per call) among the selected non-missing values of projection column
        `col` in isless order, and the counts (not missing, missing, NaN) of the selected rows"""
        ranks = np.ascontiguousarray(ranks, np.int64).reshape(-1)
        dt = self.coltype(col) & ir.DTYPE_MASK
        isf = dt in (ir.F32, ir.F64)
        out = np.zeros(len(ranks), np.float64 if isf else np.int64)
        cnt = np.zeros(3, np.int64)
        for lo in range(0, max(len(ranks), 1), 16):
            r, o = ranks[lo:lo + 16], out[lo:lo + 16]
            N.check(N.load().dfdb_order_statistics(self._h, col, r.ctypes.data if len(r) else None, len(r), None if isf else o.ctypes.data,
                                                   o.ctypes.data if isf else None, cnt.ctypes.data))
        if dt in (ir.U8, ir.U16, ir.U32, ir.U64):
            out = out.view(np.uint64)
        elif dt == ir.BOOL:
            out = out != 0
        return out, (int(cnt[0]), int(cnt[1]), int(cnt[2]))

    def sort_indices(self, col: int = 0, rev: bool = False, limit: Optional[int] = None, dev_ptr: Optional[int] = None, cap: Optional[int] = None):
        """dfdb_sort_indices: (rows, info) — the 1-based table rows of the selected rows in the stable order of projection column `col` (rev: descending;
        ties keep ascending row order both ways; missing rows last, first under rev), cut to the first `limit`; info = (selected rows, pairs sorted,
        digit passes run, digit passes skipped).  dev_ptr: write into device memory holding `cap` entries instead, without a count: (None, info)"""
        L, flags = N.load(), (N.SORT_REV if rev else 0)
        return self._sorted_rows(lambda *out: L.dfdb_sort_indices(self._h, col, flags, *out), limit, dev_ptr, cap)

    def _sorted_rows(self, sort, limit, dev_ptr, cap):
        """sort(limit, out, cap, memkind, n, info) — the tail of both sort entry points — into device memory at dev_ptr (`cap` entries, no count read back) or
        into a host array of the count: (rows or None, info)"""
        lim = -1 if limit is None else int(limit)
        info = np.zeros(4, np.int64)
        if dev_ptr is not None:
            N.check(sort(lim, C.c_void_p(dev_ptr), int(cap), N.MEM_DEVICE, None, info.ctypes.data))
            return None, tuple(int(x) for x in info)
        n = self.count() if lim < 0 else min(lim, self.count())
        out = np.empty(n, np.int64)
        got = C.c_int64()
        N.check(sort(lim, out.ctypes.data if n else None, n, N.MEM_HOST, C.byref(got), info.ctypes.data))
        return out[:got.value], tuple(int(x) for x in info)

    def sort_indices_n(self, cols, revs=None, limit: Optional[int] = None, dev_ptr: Optional[int] = None, cap: Optional[int] = None):
        """dfdb_sort_indices_n: (rows, info) — the 1-based table rows of the selected rows in the lexicographic order of projection columns cols[0] (major)
        .. cols[-1] (most minor); revs: one bool per column (None: all ascending).  Every key orders as sort_indices orders it, rows equal in every key keep
        ascending row order; info = (selected rows, pairs keyed, digit passes run, digit passes skipped), the last three summed over the keys.  dev_ptr / cap
        as sort_indices takes them"""
        L = N.load()
        ci = np.ascontiguousarray(cols, np.int32).reshape(-1)
        fl = np.zeros(len(ci), np.int32) if revs is None else np.array([N.SORT_REV if r else 0 for r in revs], np.int32)
        if len(fl) != len(ci):
            raise ValueError(f"ArgumentError: {len(fl)} rev flags for {len(ci)} sort columns")
        return self._sorted_rows(lambda *out: L.dfdb_sort_indices_n(self._h, ci.ctypes.data, fl.ctypes.data, len(ci), *out), limit, dev_ptr, cap)

    def sort_indices_any(self, cols, revs=None, limit: Optional[int] = None, dev_ptr: Optional[int] = None, cap: Optional[int] = None):
        """dfdb_sort_indices_any: sort_indices_n with String keys admitted — any key may be a plain String column (bytes compared unsigned, the shorter of two
        strings that tie is smaller; missing last, first under rev), of at most SORT_MAX_STRING_BYTES bytes per selected live row.  A String key is m + 1
        sub-keys of 8 bytes on the device and info's last three entries are summed over keys and sub-keys; with a String key `limit` only cuts what comes
        back.  With numeric keys only it is sort_indices_n"""
        L = N.load()
        ci = np.ascontiguousarray(cols, np.int32).reshape(-1)
        fl = np.zeros(len(ci), np.int32) if revs is None else np.array([N.SORT_REV if r else 0 for r in revs], np.int32)
        if len(fl) != len(ci):
            raise ValueError(f"ArgumentError: {len(fl)} rev flags for {len(ci)} sort columns")
        return self._sorted_rows(lambda *out: L.dfdb_sort_indices_any(self._h, ci.ctypes.data, fl.ctypes.data, len(ci), *out), limit, dev_ptr, cap)

    def _string_keys(self, cols) -> bool:
        """whether one of the projection columns `cols` is a String column: the sorts over it go through sort_indices_any"""
        return any((self.coltype(int(c)) & ir.DTYPE_MASK) == ir.STRING for c in cols)

    @staticmethod
    def _rows_arg(rows, dev_ptr, n):
        """(n, pointer, memkind) of 1-based table rows: a list on the host (the pointer keeps its array alive), or `n` of them in device memory at dev_ptr"""
        if dev_ptr is not None:
            return int(n), C.c_void_p(dev_ptr), N.MEM_DEVICE
        rows = np.ascontiguousarray(rows, np.int64).reshape(-1)
        return len(rows), (rows.ctypes.data_as(C.c_void_p) if len(rows) else None), N.MEM_HOST

    def gather_rows(self, rows=None, dev_ptr: Optional[int] = None, n: Optional[int] = None) -> List[Any]:
        """dfdb_gather_rows: the view's (fixed-width) projection columns at the 1-based table `rows`, in that order — any order, repeats allowed, whatever the
        selection; nullable columns come back masked.  dev_ptr / n: the rows lie in device memory (the device output of sort_indices)"""
        n, ptr, kind = self._rows_arg(rows, dev_ptr, n)
        return self._columns_out(n, lambda outs, ncols: N.check(N.load().dfdb_gather_rows(self._h, ptr, n, kind, outs, ncols)))

    def gather_rows_string_bytes(self, col: int, rows=None, dev_ptr: Optional[int] = None, n: Optional[int] = None) -> int:
        """dfdb_gather_rows_string_bytes: the string bytes projection column `col` needs at the 1-based table `rows` (0 for a fixed-width column)"""
        n, ptr, kind = self._rows_arg(rows, dev_ptr, n)
        nb = C.c_int64()
        N.check(N.load().dfdb_gather_rows_string_bytes(self._h, col, ptr, n, kind, C.byref(nb)))
        return nb.value

    def gather_rows_any(self, rows=None, dev_ptr: Optional[int] = None, n: Optional[int] = None) -> List[Any]:
        """dfdb_gather_rows_any: gather_rows for every plain column of the view, String columns included: a String column comes back as (int32 sizes with -1
        for missing, concatenated bytes) in the order of `rows`, as materialize returns it, its buffer sized by dfdb_gather_rows_string_bytes; a nullable
        fixed-width column comes back masked.  dev_ptr / n: the rows lie in device memory"""
        L = N.load()
        n, ptr, kind = self._rows_arg(rows, dev_ptr, n)

        def string_bytes(i):
            nb = C.c_int64()
            N.check(L.dfdb_gather_rows_string_bytes(self._h, i, ptr, n, kind, C.byref(nb)))
            return nb.value

        return self._columns_out(n, lambda outs, ncols: N.check(L.dfdb_gather_rows_any(self._h, ptr, n, kind, outs, ncols)), string_bytes)

    def join_count(self, other: "_Query", col: int, other_col: int, kind: int = N.JOIN_INNER):
        """dfdb_query_join: (npairs, info) of the join of this query's selected rows (the left side) with `other`'s on projection columns col / other_col;
        info = (selected left rows, selected right rows, left rows with a missing key, right rows with a missing key, digit passes run on the right side).
        The lists stay pending in this query until join_fetch; `other` is not needed for it"""
        n = C.c_int64()
        info = np.zeros(5, np.int64)
        N.check(N.load().dfdb_query_join(self._h, int(col), other._h, int(other_col), int(kind), C.byref(n), info.ctypes.data))
        return n.value, tuple(int(x) for x in info)

    def join_count_n(self, other: "_Query", cols, other_cols, kind: int = N.JOIN_INNER):
        """dfdb_query_join_n: join_count on several key columns per side (projection columns, the major key first; String keys are admitted); info =
        (selected left rows, selected right rows, left / right rows with a missing component, digit passes run on the right side, sub-keys refined).
        The lists stay pending in this query until join_fetch"""
        lc, rc = np.ascontiguousarray(cols, np.int32), np.ascontiguousarray(other_cols, np.int32)
        if lc.ndim != 1 or lc.shape != rc.shape:
            raise ValueError(f"ArgumentError: {lc.size} left and {rc.size} right key columns")
        n = C.c_int64()
        info = np.zeros(6, np.int64)
        N.check(N.load().dfdb_query_join_n(self._h, lc.ctypes.data, other._h, rc.ctypes.data, int(lc.size), int(kind), C.byref(n), info.ctypes.data))
        return n.value, tuple(int(x) for x in info)

    def join_fetch(self, npairs: int, dev_ptrs=None, want_right: bool = True):
        """dfdb_query_join_fetch of the pending join: (left_rows, right_rows) as host arrays of npairs 1-based table rows (right_rows None unless wanted; 0 in
        it: no match), or — dev_ptrs = (left pointer, right pointer or None), each holding npairs entries of device memory — written there: (None, None)"""
        L = N.load()
        if dev_ptrs is not None:
            lp, rp = dev_ptrs
            N.check(L.dfdb_query_join_fetch(self._h, C.c_void_p(lp), C.c_void_p(rp) if rp else None, int(npairs), N.MEM_DEVICE))
            return None, None
        lr = np.empty(npairs, np.int64)
        rr = np.empty(npairs, np.int64) if want_right else None
        N.check(L.dfdb_query_join_fetch(self._h, lr.ctypes.data if npairs else None, rr.ctypes.data if (want_right and npairs) else None, int(npairs), N.MEM_HOST))
        return lr, rr

    def join(self, other: "_Query", col, other_col, kind: int = N.JOIN_INNER, device: bool = False):
        """both calls: (left_rows, right_rows, info) — two parallel lists of 1-based table rows ordered by left row, then by right row; right_rows[i] = 0: no
        match.  col / other_col: one projection column each (dfdb_query_join) or two lists of them (dfdb_query_join_n: several keys, String keys).
        device: the lists stay on the device, as two int64 tensors of the context's device (torch), ready for gather_rows_any(dev_ptr = ..)"""
        n, info = self.join_count(other, col, other_col, kind) if isinstance(col, (int, np.integer)) else self.join_count_n(other, col, other_col, kind)
        if not device:
            return self.join_fetch(n) + (info,)
        import torch
        dev = torch.device("cuda", self.view.table.ctx.device)
        lt, rt = torch.empty(max(n, 1), dtype=torch.int64, device=dev), torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        self.join_fetch(n, (lt.data_ptr(), rt.data_ptr()))
        return lt[:n], rt[:n], info


class _ChunkQuery(_Query):
    """One chunk of a streamed view: the engine owns the handle (valid until the stream advances)."""

    def __init__(self, view: DFView, handle, chunk_rows: int, first_row: int):
        self.view, self._h, self.chunk_rows, self.first_row = view, handle, chunk_rows, first_row

    def __del__(self):
        pass

    def bitmap(self) -> np.ndarray:
        out = np.zeros((self.chunk_rows + 63) // 64, np.uint64)
        if len(out):
            N.check(N.load().dfdb_select_bitmap(self._h, out.ctypes.data, N.MEM_HOST))
        return out


DEFAULT_CHUNK_BLOCKS = 512      # blocks per chunk of the block-streamed consumers that open their own Stream (unique, aggregates, groupreduce over a table that is not resident)


class Stream:
    """Base.iterate(::BlocksIterator) in chunks of blocks (blocksiterator.jl:98-145) for a view over a table that was opened
    with load=False: `for part in dfdb.stream(v, chunk_blocks=256): part.count(), part.indices(), part.materialize()`.
    The next chunk is read, copied and LZ4-decoded on another HIP stream while the caller works on the current one."""

    def __init__(self, v: Union[DFView, DFTable], chunk_blocks: Optional[int] = None):
        chunk_blocks = DEFAULT_CHUNK_BLOCKS if chunk_blocks is None else chunk_blocks
        self.view = v if isinstance(v, DFView) else DFView(v)
        self._q = _Query(self.view)
        self._h = C.c_void_p()
        N.check(N.load().dfdb_stream_open(self._q._h, chunk_blocks, C.byref(self._h)))

    def stats(self) -> dict:
        st = N.SizeStats()
        N.check(N.load().dfdb_stream_stats(self._h, C.byref(st)))
        return {"rows": st.rows, "compressed": st.compressed, "uncompressed": st.uncompressed}

    def read_stats(self, column: Optional[str] = None) -> dict:
        """what the loaders have read so far of one column (None: of every required column): late materialization reads a projection-only
        column only for the blocks whose selection kept a row (blocksiterator.jl:111-113)"""
        st = N.SizeStats()
        o = -1 if column is None else self.view.table.names().index(column)
        N.check(N.load().dfdb_stream_read_stats(self._h, o, C.byref(st)))
        return {"rows": st.rows, "compressed": st.compressed, "uncompressed": st.uncompressed}

    def __iter__(self):
        return self

    def __next__(self) -> _ChunkQuery:
        if not self._h:
            raise StopIteration
        h, rows, first = C.c_void_p(), C.c_int64(), C.c_int64()
        N.check(N.load().dfdb_stream_next(self._h, C.byref(h), C.byref(rows), C.byref(first)))
        if not h:
            self.close()
            raise StopIteration
        return _ChunkQuery(self.view, h, rows.value, first.value)

    def close(self):
        if self._h:
            N.load().dfdb_stream_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def __del__(self):
        try:
            import sys
            if not sys.is_finalizing():
                self.close()
        except Exception:
            pass


def stream(v: Union[DFView, DFTable], chunk_blocks: int = 512) -> Stream:
    return Stream(v, chunk_blocks)


def _with_chunk_blocks(view: "DFView", chunk_blocks: Optional[int]):
    if chunk_blocks is not None:
        view.table.ctx.set_option("ooc_chunk_blocks", int(chunk_blocks))


def nrow_streamed(v: Union[DFView, DFTable], chunk_blocks: Optional[int] = None) -> int:
    """nrow(v) without holding the table in HBM (BlockRowsIterator, view.jl:192-206): ONE call — dfdb_count notices that the view's columns are not
    resident and streams the selection's columns (the first projection column when there is no predicate) inside the library (csrc/ooc.cpp)."""
    view = v if isinstance(v, DFView) else DFView(v)
    _with_chunk_blocks(view, chunk_blocks)
    return nrow(view)


def materialize_streamed(v: Union[DFView, DFTable], chunk_blocks: Optional[int] = None):
    """materialize(v) over a table that is not resident: dfdb_count + dfdb_materialize stream inside the library, every chunk's rows appended to the
    caller's buffers (materialization.jl:33-37)."""
    view = v if isinstance(v, DFView) else DFView(v)
    _with_chunk_blocks(view, chunk_blocks)
    return materialize(view)


def _flat_to_strings(sizes: np.ndarray, data: np.ndarray) -> List[Optional[str]]:
    out, o = [], 0
    raw = data.tobytes()
    for s in sizes.tolist():
        if s < 0:
            out.append(None)
        else:
            out.append(raw[o:o + s].decode(errors="replace"))
            o += s
    return out


# String columns come back from the engine as (Int32 sizes, byte arena) — a FlatStringsVector.  "object": one Python str per row like the
# reference's Vector{String} (projection.jl:99-100; ~0.2 us per row in the interpreter); "arrow": the same two buffers wrapped as a
# pyarrow large_string array inside a pandas ArrowExtensionArray — no per-row work, missing rows are nulls.
_STRING_OUTPUT = "object"


def set_string_output(kind: str) -> None:
    global _STRING_OUTPUT
    if kind not in ("object", "arrow"):
        raise ValueError("string output is 'object' or 'arrow'")
    _STRING_OUTPUT = kind


def _flat_to_arrow(sizes: np.ndarray, data: np.ndarray):
    import pyarrow as pa
    sizes = np.asarray(sizes, np.int32)
    off = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(np.where(sizes > 0, sizes, 0), out=off[1:])
    valid = np.packbits(sizes >= 0, bitorder="little")
    return pa.Array.from_buffers(pa.large_string(), len(sizes), [pa.py_buffer(valid), pa.py_buffer(off), pa.py_buffer(np.ascontiguousarray(data, np.uint8))])


# ---------------------------------------------------------------- nrow / size / materialize
def nrow(v: Union[DFView, DFTable, "DFColumn"]) -> int:      # view.jl:192-206
    if isinstance(v, DFTable):
        v = DFView(v)
    if isinstance(v, DFColumn):
        v = v.view
    if len(v.projection) == 0:
        return 0      # isempty(it.streams): nothing to read, zero rows (blocksiterator.jl:101)
    return v._query().count()      # (a view over columns that are not resident is block-streamed inside dfdb_count: csrc/ooc.cpp)


def _out_of_core(v: DFView) -> bool:
    """The view touches a column of a file-backed table that is not resident (open_table(path, load=False)): the library evaluates it
    block-streamed, the way the reference always does (blocksiterator.jl:98-145).  Informational: nothing here routes on it any more."""
    t = v.table
    if not t.path:
        return False
    need = set(v.required_columns()) or set(t.names()[:1])
    return any(not t.resident(t.ordinal(n)) for n in need)


def ncol(v: Union[DFView, DFTable]) -> int:
    return len((v if isinstance(v, DFView) else DFView(v)).projection)


def size(v, dim: Optional[int] = None):
    if isinstance(v, DFColumn):
        return (nrow(v),) if dim is None else (nrow(v) if dim == 1 else 1)
    if dim is None:
        return (nrow(v), ncol(v))
    if dim not in (1, 2):
        raise ValueError("ArgumentError: DFView have only 2 dimensions")
    return nrow(v) if dim == 1 else ncol(v)


def materialize(v: Union[DFView, DFTable, "DFColumn"]):
    """materialize(::DFView) -> pandas.DataFrame (stand-in for DataFrames.DataFrame); materialize(::DFColumn) -> array."""
    if isinstance(v, DFColumn):
        cols = v.view._query().materialize()
        return _to_user(cols[0], _logicals(v.view)[0])
    if isinstance(v, DFTable):
        v = DFView(v)
    import pandas as pd
    cols = v._query().materialize() if len(v.projection) else []
    lg = _logicals(v)
    return pd.DataFrame({k: _to_user(c, lg[i]) for i, (k, c) in enumerate(zip(v.projection.keys(), cols))})


def _logicals(v: DFView) -> List[str]:
    """per projection column: the bits type its values stand for, as the engine types the expression ("" for ordinary dtypes)"""
    metas = None
    out = []
    for e in v.projection.cols.values():
        if e.op == ir.COL:
            metas = metas or v.table.columns_meta()
            out.append(metas[e.payload].logical)
        else:
            out.append(v.table.expr_logical(e))
    return out


def _to_user(c, logical: str = ""):
    if isinstance(c, tuple):
        if _STRING_OUTPUT == "arrow":
            import pandas as pd
            return pd.arrays.ArrowExtensionArray(_flat_to_arrow(*c))
        return np.array(_flat_to_strings(*c), dtype=object)
    if logical:
        if isinstance(c, np.ma.MaskedArray):
            return np.ma.masked_array(ir.from_logical(np.asarray(c.data), logical), mask=np.ma.getmaskarray(c))
        return ir.from_logical(c, logical)
    return c


def head(v, rows: int = 10):      # materialization.jl:64-66
    v = v if isinstance(v, DFView) else DFView(v)
    return materialize(v[jr(1, rows), ALL])


# ---------------------------------------------------------------- DFColumn (column.jl:30-126, columnbroadcast.jl)
class DFColumn:
    def __init__(self, view: DFView):
        if len(view.projection) != 1:
            raise ValueError("ArgumentError: Column projection must contains singe element")
        self.view = view
        self._dtype: Optional[int] = None

    @property
    def expr(self) -> ir.Expr: return next(iter(self.view.projection.cols.values()))

    @property
    def eltype(self) -> int:
        if self._dtype is None:
            self._dtype = self.view.table.expr_dtype(self.expr)
        return self._dtype

    def _as_expr(self) -> ir.Expr: return self.expr

    def __len__(self): return nrow(self.view)
    def __eq_view__(self, o): return isinstance(o, DFColumn) and self.view == o.view

    def __getitem__(self, i):
        if isinstance(i, DFColumn):      # column.jl:63-67
            if not self.view.selection.same(i.view.selection):
                raise ValueError("ArgumentError: cols must have same selections")
            return DFColumn(self.view._selection(i))
        if isinstance(i, (int, np.integer)):
            return DFColumn(self.view._selection(int(i)))._scalar(i)
        if isinstance(i, _End):
            return self[i.resolve(len(self))]
        return DFColumn(self.view._selection(i))

    def _scalar(self, i=None):             # column.jl:93-99
        vals = self.view._query().materialize()[0]
        vals = _to_user(vals)
        if len(vals) == 0:
            raise IndexError(f"BoundsError: attempt to access column at index [{i}]")
        return vals[0]

    def materialize(self): return materialize(self)
    def collect(self): return materialize(self)
    def __iter__(self): return iter(materialize(self))

    def copyto(self, dest: np.ndarray):    # Base.copyto!(dest, src::DFColumn) (column.jl:83-91)
        vals = materialize(self)
        dest[:len(vals)] = vals
        return dest

    def unique(self):
        """unique(col) (docs/src/index.md:171-182): the distinct values in order of first appearance.  On the device the
        first occurrences are a selection (dfdb_query_unique); over a table that is not resident the same call reduces every chunk on the
        device and merges the (small) per-chunk results in order inside the library (csrc/ooc.cpp)."""
        def one(q):
            q.hint_materialize(True)
            q.execute()
            N.check(N.load().dfdb_query_unique(q._h, 0))
            return _to_user(q.materialize()[0], _logicals(self.view)[0])
        return one(self.view._query())

    def _aggregate(self, op: int, with_count: bool = False):
        """sum / min / max driven by Base.iterate(::DFColumn) in the reference (column.jl:102-126).  Over a table that is not resident
        every chunk is reduced on the device and the per-chunk results are combined in block order — inside dfdb_aggregate (csrc/ooc.cpp)."""
        # sum(f.(cols)) of a computed Bool column — `sum(ismissing.(t.col))`, docs/src/index.md:326-328 — is the number of selected rows for
        # which it holds: one more predicate on the selection (routed to the scan kernels like any other) instead of a materialised
        # Bool per row and a reduction over it
        if op == N.AGG_SUM and self.eltype == ir.BOOL and self.expr.op != ir.COL:
            cnt = nrow(DFView(self.view.table, self.view.projection, self.view.selection.add(self.expr)))
            return (cnt, nrow(self.view)) if with_count else cnt
        q = self.view._query()
        q.hint_aggregate(op)                           # before anything executes the selection
        r = q.aggregate(op)                            # (not resident: per-chunk reductions folded in block order inside the library)
        return (r, q.count()) if with_count else r

    def sum(self): return self._aggregate(N.AGG_SUM)
    def min(self): return self._aggregate(N.AGG_MIN)
    def max(self): return self._aggregate(N.AGG_MAX)

    def mean(self):
        s, n = self._aggregate(N.AGG_SUM, with_count=True)      # one evaluation of the selection gives both
        return float("nan") if n == 0 else s / n

    # -- order statistics: Statistics.median / quantile, which the reference answers by collecting Base.iterate(::DFColumn) (column.jl:102-126) and sorting;
    # here the device selects the one or two values a result is made of (dfdb_order_statistics, csrc/k_select.hip)
    def order_statistics(self, ranks):
        """(values, (n, missing, nan)): the values at the 1-based `ranks` among the n non-missing selected values in isless order (integers by value,
        floats -Inf .. -0.0 < 0.0 .. Inf < NaN; Float32 widened to Float64), and how many selected rows are not missing, missing, NaN"""
        return self.view._query().order_statistics(ranks)

    def _ordered_counts(self, q):
        """(n, missing) before any rank is known: the selection's own count when nothing can be missing, else one counting pass"""
        if self.eltype & ir.NULLABLE:
            n, nmiss, _ = q.order_statistics([])[1]
            return n, nmiss
        return q.count(), 0

    def median(self):
        """Statistics.median(col): None (missing) if a selected row is missing, NaN if one is NaN, else middle(v[mid]) for odd n and
        middle(v[mid], v[mid + 1]) = v[mid] / 2 + v[mid + 1] / 2 for even n, mid = (1 + n) ÷ 2; Float32 for a Float32 column, else Float64"""
        q = self.view._query()
        n, nmiss = self._ordered_counts(q)
        if nmiss:
            return None
        if n == 0:
            raise ValueError("ArgumentError: median of an empty array is undefined")
        mid = (1 + n) // 2
        v, (_, _, nnan) = q.order_statistics([mid] if n % 2 else [mid, mid + 1])
        F = np.float32 if (self.eltype & ir.DTYPE_MASK) == ir.F32 else np.float64
        if nnan:
            return F("nan")
        with np.errstate(all="ignore"):
            x = [F(int(e)) if v.dtype.kind in "iub" else F(e) for e in v]
            return x[0] if n % 2 else x[0] / F(2) + x[1] / F(2)

    def quantile(self, p):
        """Statistics.quantile(col, p) with the default parameters (alpha = beta = 1): aleph = n p + (1 - p), j = clamp(floor(aleph), 1, n - 1),
        gamma = clamp(aleph - j, 0, 1), a = v[j], b = v[j + 1]: a + gamma (b - a) when both are finite, else (1 - gamma) a + gamma b; Float64.
        A vector of p gives a vector."""
        ps = np.atleast_1d(np.asarray(p, np.float64))
        if not np.all((ps >= 0) & (ps <= 1)):
            raise ValueError("ArgumentError: input probability out of [0,1] range")
        q = self.view._query()
        n, nmiss = self._ordered_counts(q)
        if nmiss:
            raise ValueError("ArgumentError: quantiles are undefined in presence of missing values")
        if n == 0:
            raise ValueError("ArgumentError: empty data vector")
        js = [1 if n == 1 else min(max(int(np.floor(n * x + (1 - x))), 1), n - 1) for x in ps]
        v, (_, _, nnan) = q.order_statistics([r for j in js for r in ((j,) if n == 1 else (j, j + 1))])
        if nnan:
            raise ValueError("ArgumentError: quantiles are undefined in presence of NaNs")
        v = [float(int(e)) if v.dtype.kind in "iub" else float(e) for e in v]
        out = np.empty(len(ps), np.float64)
        with np.errstate(all="ignore"):
            for k, (x, j) in enumerate(zip(ps, js)):
                if n == 1:
                    out[k] = v[k]
                    continue
                a, b = np.float64(v[2 * k]), np.float64(v[2 * k + 1])
                g = min(max(n * x + (1 - x) - j, 0.0), 1.0)
                out[k] = a + g * (b - a) if np.isfinite(a) and np.isfinite(b) else (1 - g) * a + g * b
        return float(out[0]) if np.ndim(p) == 0 else out

    # -- ordering: sortperm / partialsortperm / sort, which the reference answers by collecting Base.iterate(::DFColumn) (column.jl:102-126) and sorting on
    # the host; here the device sorts {key, row} pairs (dfdb_sort_indices, csrc/k_sort.hip) and gathers the values in that order (dfdb_gather_rows)
    def sortperm(self, rev: bool = False, limit: Optional[int] = None) -> np.ndarray:
        """the 1-based TABLE rows of the selected rows in sorted order (stable; rev reverses the ordering, not the ties; missing last, first under rev),
        the first `limit` of them when given"""
        q = self.view._query()
        return (q.sort_indices_any([0], [rev], limit) if q._string_keys([0]) else q.sort_indices(0, rev, limit))[0]

    def sort(self, rev: bool = False, limit: Optional[int] = None):
        """sort(collect(col); rev) — the first `limit` values of it when given —, missing values as materialize gives them"""
        q = self.view._query()
        if q._string_keys([0]):                         # a String column: sorted by its bytes (dfdb_sort_indices_any), gathered through dfdb_gather_rows_any
            rows, _ = q.sort_indices_any([0], [rev], limit)
            return _to_user(q.gather_rows_any(rows)[0], _logicals(self.view)[0])
        rows, _ = q.sort_indices(0, rev, limit)
        return _to_user(q.gather_rows(rows)[0], _logicals(self.view)[0])

    # -- broadcasting (columnbroadcast.jl:19-62): every DFColumn argument must share (table, selection)
    def _bc(self, op: int, other, swap: bool = False) -> "DFColumn":
        if isinstance(other, DFColumn):
            if not (self.view.table == other.view.table and self.view.selection.same(other.view.selection)):
                raise ValueError("ArgumentError: All columns in broadcast must have same selection and table")
        elif isinstance(other, (list, tuple, np.ndarray)):
            raise TypeError("broadcasting a DFColumn with an array falls back to array style in the reference (columnbroadcast.jl:16-17)")
        a, b = ir.wrap(self), ir.wrap(other)
        e = ir.Expr(op, (b, a) if swap else (a, b))
        return DFColumn(DFView(self.view.table, Projection({"a": e}), self.view.selection))

    def _un(self, op: int) -> "DFColumn":
        return DFColumn(DFView(self.view.table, Projection({"a": ir.Expr(op, (self.expr,))}), self.view.selection))

    def __add__(self, o): return self._bc(ir.ADD, o)
    def __radd__(self, o): return self._bc(ir.ADD, o, True)
    def __sub__(self, o): return self._bc(ir.SUB, o)
    def __rsub__(self, o): return self._bc(ir.SUB, o, True)
    def __mul__(self, o): return self._bc(ir.MUL, o)
    def __rmul__(self, o): return self._bc(ir.MUL, o, True)
    def __truediv__(self, o): return self._bc(ir.DIV, o)
    def __rtruediv__(self, o): return self._bc(ir.DIV, o, True)
    def __mod__(self, o): return self._bc(ir.REM, o)
    def __rmod__(self, o): return self._bc(ir.REM, o, True)
    def __neg__(self): return self._un(ir.NEG)
    def __abs__(self): return self._un(ir.ABS)
    def __invert__(self): return self._un(ir.NOT)
    def __and__(self, o): return self._bc(ir.AND, o)
    def __rand__(self, o): return self._bc(ir.AND, o, True)
    def __or__(self, o): return self._bc(ir.OR, o)
    def __ror__(self, o): return self._bc(ir.OR, o, True)
    def __xor__(self, o): return self._bc(ir.XOR, o)
    def __lt__(self, o): return self._bc(ir.LT, o)
    def __le__(self, o): return self._bc(ir.LE, o)
    def __gt__(self, o): return self._bc(ir.GT, o)
    def __ge__(self, o): return self._bc(ir.GE, o)
    def __eq__(self, o): return self._bc(ir.EQ, o)     # `.==` ; use col_equal(a, b) for DFColumn == DFColumn (column.jl:39)
    def __ne__(self, o): return self._bc(ir.NE, o)
    def __hash__(self): return id(self)
    def __bool__(self): raise TypeError("a DFColumn has no truth value: use & | ~ and split chained comparisons")

    def __repr__(self): return f"DFColumn{{{ir.dtype_name(self.eltype)}}}"


def median(c: DFColumn): return c.median()                # Statistics.median(col)
def quantile(c: DFColumn, p): return c.quantile(p)        # Statistics.quantile(col, p)


def sortperm(c: DFColumn, rev: bool = False, limit: Optional[int] = None): return c.sortperm(rev, limit)      # Base.sortperm(col; rev): table rows
def sort(c: DFColumn, rev: bool = False, limit: Optional[int] = None): return c.sort(rev, limit)              # Base.sort(col; rev)
def partialsortperm(c: DFColumn, k: int, rev: bool = False): return c.sortperm(rev, k)                        # Base.partialsortperm(col, 1:k; rev)


def _sort_keys(v: DFView, by, rev):
    """(projection columns, one rev per column) of a list of column names and a bool or a list of bools"""
    names = list(v.projection.keys())
    revs = [bool(rev)] * len(by) if isinstance(rev, (bool, np.bool_)) else [bool(r) for r in rev]
    if len(revs) != len(by):
        raise ValueError(f"ArgumentError: rev has {len(revs)} entries for {len(by)} sort columns")
    return [names.index(b) for b in by], revs


def sortperm_by(v: Union[DFView, DFTable], by, rev=False, limit: Optional[int] = None) -> np.ndarray:
    """sortperm by a tuple of columns: the 1-based TABLE rows of the selected rows of `v` in the lexicographic order of its columns `by` (a name or a list of
    names, the first one major), `rev` a bool or one per column; rows equal in every key keep ascending row order"""
    if isinstance(v, DFTable):
        v = DFView(v)
    if isinstance(by, str):
        by = [by]
    cols, revs = _sort_keys(v, by, rev)
    q = v._query()
    return (q.sort_indices_any(cols, revs, limit) if q._string_keys(cols) else q.sort_indices_n(cols, revs, limit))[0]


def sort_view(v: Union[DFView, DFTable], by, rev=False, limit: Optional[int] = None):
    """sort!(materialize(v), by; rev) (first(.., limit) when given): the view's projection columns, String columns included, in the order of its column `by`,
    or of its columns `by` when that is a list of names (the first one major; `rev` a bool or one per column).  A key is a fixed-width column or a plain
    String column (sorted by its bytes, at most SORT_MAX_STRING_BYTES per selected row: dfdb_sort_indices_any); every column follows the keys through
    dfdb_gather_rows_any"""
    if isinstance(v, DFTable):
        v = DFView(v)
    import pandas as pd
    q = v._query()
    names = list(v.projection.keys())
    if q._string_keys([names.index(b) for b in ([by] if isinstance(by, str) else by)]):
        rows, _ = q.sort_indices_any(*_sort_keys(v, [by] if isinstance(by, str) else by, rev), limit)
    elif isinstance(by, str):
        rows, _ = q.sort_indices(names.index(by), rev, limit)
    else:
        rows, _ = q.sort_indices_n(*_sort_keys(v, by, rev), limit)
    lg = _logicals(v)
    return pd.DataFrame({k: _to_user(c, lg[i]) for i, (k, c) in enumerate(zip(v.projection.keys(), q.gather_rows_any(rows)))})


def take(v: Union[DFView, DFTable], rows):
    """materialize(v)'s columns at given rows: the view's projection at the 1-based TABLE `rows` — any order, repeats allowed, whatever the view selects — as a
    DataFrame (dfdb_gather_rows_any)"""
    if isinstance(v, DFTable):
        v = DFView(v)
    import pandas as pd
    lg = _logicals(v)
    return pd.DataFrame({k: _to_user(c, lg[i]) for i, (k, c) in enumerate(zip(v.projection.keys(), v._query().gather_rows_any(rows)))})


_JOIN_KINDS = {"inner": N.JOIN_INNER, "left": N.JOIN_LEFT, "semi": N.JOIN_SEMI, "anti": N.JOIN_ANTI}


def _join_sides(v, w, on):
    """(left view, right view, the left keys' projection columns, the right keys') of a join `on` a name, a (left name, right name) pair, or a list of either"""
    v = DFView(v) if isinstance(v, DFTable) else v
    w = DFView(w) if isinstance(w, DFTable) else w
    pairs = [(o, o) if isinstance(o, str) else tuple(o) for o in (on if isinstance(on, list) else [on])]
    if not pairs or any(len(p) != 2 for p in pairs):
        raise ValueError(f"ArgumentError: on = {on!r} (a column name, a (left name, right name) pair, or a list of them)")
    lnames, rnames = list(v.projection.keys()), list(w.projection.keys())
    for ln, rn in pairs:
        for name, names in ((ln, lnames), (rn, rnames)):
            if name not in names:
                raise KeyError(f"KeyError: column {name} not found")
    return v, w, [lnames.index(ln) for ln, _ in pairs], [rnames.index(rn) for _, rn in pairs]


def _join_single(v, w, lc, rc):
    """whether the join takes dfdb_query_join: one key, fixed-width on both sides (a String key and several keys take dfdb_query_join_n)"""
    if len(lc) != 1:
        return False
    q, p = v._query(), w._query()
    return (q.coltype(lc[0]) & ~ir.NULLABLE) != ir.STRING and (p.coltype(rc[0]) & ~ir.NULLABLE) != ir.STRING


def _join_call(v, w, on, kind, matchmissing):
    """call 1 of the join of two views: (left view, right view, left query, npairs, info, the right keys' columns); matchmissing = "error" raises on a missing key"""
    if kind not in _JOIN_KINDS:
        raise ValueError(f"ArgumentError: join kind {kind!r} (inner, left, semi or anti)")
    if matchmissing not in ("error", "notequal"):
        raise ValueError(f"ArgumentError: matchmissing = {matchmissing!r} (error or notequal)")
    v, w, lc, rc = _join_sides(v, w, on)
    q = v._query()
    if _join_single(v, w, lc, rc):
        n, info = q.join_count(w._query(), lc[0], rc[0], _JOIN_KINDS[kind])
    else:
        n, info = q.join_count_n(w._query(), lc, rc, _JOIN_KINDS[kind])
    if matchmissing == "error" and (info[2] or info[3]):      # (the pending lists stay until the query's next join or reset: its executed selection is kept)
        raise ValueError(f"ArgumentError: missing values in the key column{'s' if len(lc) > 1 else ''} of the {'left' if info[2] else 'right'} side ({info[2]} left, {info[3]} right rows): "
                         "pass matchmissing = \"notequal\" to let them match nothing")
    return v, w, q, n, info, rc


def join_rows(v, w, on, kind: str = "inner", matchmissing: str = "error"):
    """The row lists of innerjoin / leftjoin / semijoin / antijoin of two views (dfdb_query_join; several keys or a String key: dfdb_query_join_n):
    (left_rows, right_rows, info) — parallel arrays of 1-based TABLE rows ordered by left row, then by right row; right_rows[i] = 0: no match (kind "left" and
    "anti").  `on`: a column name, a (left name, right name) pair, or a list of either (the major key first).  Keys compare with isequal; matchmissing = "error" (DataFrames.jl's default) raises ValueError when a selected key is missing on
    either side, "notequal" lets such a row match nothing.  info: (selected left rows, selected right rows, left / right rows with a missing key, digit passes)
    for a single fixed-width key; with several keys or a String key those five — a row with ANY component missing counted once — and a sixth, the 8-byte
    sub-keys refined (dfdb_query_join_n's info[6])"""
    _, _, q, n, info, _ = _join_call(v, w, on, kind, matchmissing)
    return q.join_fetch(n) + (info,)


def _join_frame(v, w, on, kind, matchmissing):
    import pandas as pd
    import torch
    v, w, _, rc = _join_sides(v, w, on)
    lnames, rnames = list(v.projection.keys()), list(w.projection.keys())
    rkeep = [i for i in range(len(rnames)) if i not in rc] if kind == "inner" else []
    dup = [rnames[i] for i in rkeep if rnames[i] in lnames]
    if dup:                                                   # (before anything runs, as DataFrames.jl checks its names)
        raise ValueError(f"ArgumentError: Duplicate variable names: {', '.join(dup)}. Pass makeunique=true to make them unique")
    v, w, q, n, info, rc = _join_call(v, w, on, kind, matchmissing)
    dev = torch.device("cuda", v.table.ctx.device)
    lt = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    rt = torch.empty(max(n, 1), dtype=torch.int64, device=dev) if rkeep else None
    q.join_fetch(n, (lt.data_ptr(), rt.data_ptr() if rkeep else None))
    lg = _logicals(v)
    cols = {k: _to_user(c, lg[i]) for i, (k, c) in enumerate(zip(lnames, q.gather_rows_any(dev_ptr=lt.data_ptr(), n=n)))}
    if rkeep:
        rg = _logicals(w)
        rcols = w._query().gather_rows_any(dev_ptr=rt.data_ptr(), n=n)
        cols.update({rnames[i]: _to_user(rcols[i], rg[i]) for i in rkeep})
    return pd.DataFrame(cols)


def innerjoin(v, w, on, matchmissing: str = "error"):
    """innerjoin(materialize(v), materialize(w); on) as a DataFrame: the left view's columns, then the right view's without its key columns, one row per match, ordered
    by left row then right row.  The row lists stay on the device (dfdb_query_join_fetch into device memory) and both sides are gathered from them with
    dfdb_gather_rows_any.  A non-key name present on both sides is an ArgumentError (makeunique = false)"""
    return _join_frame(v, w, on, "inner", matchmissing)


def semijoin(v, w, on, matchmissing: str = "error"):
    """semijoin: the left view's columns at its selected rows that have a match in `w`, in table order"""
    return _join_frame(v, w, on, "semi", matchmissing)


def antijoin(v, w, on, matchmissing: str = "error"):
    """antijoin: the left view's columns at its selected rows that have no match in `w`, in table order"""
    return _join_frame(v, w, on, "anti", matchmissing)


def col_equal(a: DFColumn, b: DFColumn) -> bool:
    """Base.:(==)(a::DFColumn, b::DFColumn) = a.view == b.view (column.jl:39)."""
    return a.view == b.view


def _fn_bc(maker):
    def f(c, *args):
        if isinstance(c, DFColumn):
            e = maker(c.expr, *args)
            return DFColumn(DFView(c.view.table, Projection({"a": e}), c.view.selection))
        return maker(c, *args)
    return f


startswith = _fn_bc(ir.startswith)
endswith = _fn_bc(ir.endswith)
ismissing = _fn_bc(ir.ismissing)
isin = _fn_bc(ir.isin)
sizeof = _fn_bc(ir.sizeof)
float64 = _fn_bc(ir.float64)


def parse(dtype: int, c):
    """parse.(T, col): a String column (or Expr) as an integer type or Float64; the result type is the engine's (dfdb_expr_result_type): T, never missing."""
    return _fn_bc(lambda e: ir.parse(dtype, e))(c)


datetime19 = _fn_bc(ir.datetime19)
datetime19.__doc__ = """datetime19.(col): a String column of "yyyy-mm-dd HH:MM:SS…" timestamps as a DateTime column (ir.datetime19)."""


def coalesce(c, default):
    """coalesce.(col, default): DFColumn or Expr; `default` may itself be a column of the same view."""
    if isinstance(c, DFColumn):
        d = default.expr if isinstance(default, DFColumn) else default
        return DFColumn(DFView(c.view.table, Projection({"a": ir.coalesce(c.expr, d)}), c.view.selection))
    return ir.coalesce(c, default)


def string(c):
    """string.(col) over a String column: coalesce.(col, "missing") where the column is Union{String,Missing} (Julia's string(missing)), the column itself
    where it is a plain String column.  An Expr carries no type: it is taken as nullable, which gives a plain column back unchanged too."""
    if isinstance(c, DFColumn):
        if (c.eltype & ir.DTYPE_MASK) != ir.STRING:
            raise NotImplementedError(f"string.(col) over {ir.dtype_name(c.eltype)} is not built: String columns only")
        return coalesce(c, "missing") if c.eltype & ir.NULLABLE else c
    return ir.string(c)


def view_from_columns(**cols: DFColumn) -> DFView:
    """DFView(a = col1, g = col2) (column.jl:143-164)."""
    first = None
    for c in cols.values():
        if first is None:
            first = c
        elif not (c.view.table == first.view.table and c.view.selection.same(first.view.selection)):
            raise ValueError("ArgumentError: All columns must have same selection and table")
    if first is None:
        raise ValueError("ArgumentError: no columns")
    return DFView(first.view.table, Projection({k: c.expr for k, c in cols.items()}), first.view.selection)


def table_stats(t: DFTable):
    """table_stats(table) (misc.jl:6-43): rows, uncompressed and compressed size and ratio per column + the table total, from the
    block headers of the column files (numbers, not the reference's pretty-printed strings)."""
    import pandas as pd
    rows = []
    tot = [0, 0, 0]
    for i, m in enumerate(t.columns_meta()):
        st = N.SizeStats()
        N.check(N.load().dfdb_table_column_stats(t._h, i, C.byref(st)))
        rows.append((m.name, m.type, st.rows, st.uncompressed, st.compressed, st.uncompressed / st.compressed if st.compressed else float("nan")))
        tot = [st.rows, tot[1] + st.uncompressed, tot[2] + st.compressed]
    if rows:
        rows.append(("Table total", "", tot[0], tot[1], tot[2], tot[1] / tot[2] if tot[2] else float("nan")))
    return pd.DataFrame(rows, columns=["column", "type", "rows", "uncompressed size", "compressed size", "compression ratio"])


def create_table(path: str, from_=None, block_size: int = 65536, ctx: Optional[Context] = None, **columns) -> "DFTable":
    """create_table(path; from=..., block_size=...) (creators.jl:18-60).  `from_`: a dict of host columns, a DFTable, or a
    DFView / DFColumn(s) to materialise (on the device) first.  Writes the table directory and returns the opened table."""
    src = from_ if from_ is not None else columns
    if isinstance(src, DFTable):
        t = src
    elif isinstance(src, (DFView, DFColumn)):
        v = src.view if isinstance(src, DFColumn) else src
        t = DFTable.new(block_size=block_size, ctx=v.table.ctx)
        for name in v.names():
            t.add_column_from(name, v[ALL, name])
    else:
        t = DFTable.from_columns(dict(src), block_size=block_size, ctx=ctx)
    t.save(path)
    return open_table(path, ctx=t.ctx)


def map_to_column(f: Callable, v: Union[DFView, DFTable]) -> DFColumn:   # view.jl:160-164
    v = v if isinstance(v, DFView) else DFView(v)
    return v[ALL, (tuple(v.names()), f)]


# ---------------------------------------------------------------- groupreduce (aggregate.jl:1-36, completed to its evident intent)
_STATS = {"count": N.AGG_COUNT, "sum": N.AGG_SUM, "min": N.AGG_MIN, "minimum": N.AGG_MIN, "max": N.AGG_MAX, "maximum": N.AGG_MAX, "mean": N.AGG_SUM}


def _groupreduce_view(v: Union[DFView, DFTable], by: str, col: Optional[str], stat: str):
    v = v if isinstance(v, DFView) else DFView(v)
    if stat not in _STATS:
        raise ValueError(f"ArgumentError: unknown statistic {stat}")
    names = [by] if col is None or stat == "count" else [by, col]
    return (v[ALL, names] if len(names) > 1 else DFView(v.table, Projection({by: v.projection.cols[by]}), v.selection)), len(names) > 1


def _groupreduce_raw(q: "_Query", with_value: bool, stat: str):
    """dfdb_query_groupreduce + _fetch on one query handle -> (keys, counts, values as Int64 bits, values as Float64, value dtype or None);
    keys are a numpy array, a masked array (nullable key) or a list of str / None."""
    L = N.load()
    ng, kb = C.c_int64(), C.c_int64()
    N.check(L.dfdb_query_groupreduce(q._h, 0, 1 if with_value else -1, _STATS[stat], C.byref(ng), C.byref(kb)))
    n = ng.value
    kdt = q.coltype(0)
    out = N.OutCol()
    out.memkind = N.MEM_HOST
    if (kdt & ir.DTYPE_MASK) == ir.STRING:
        ksz = np.empty(max(n, 1), np.int32); kby = np.empty(max(kb.value, 1), np.uint8)
        out.data, out.bytes, out.bytes_cap = ksz.ctypes.data, kby.ctypes.data, kb.value
    else:
        karr = np.empty(max(n, 1), ir.numpy_of_dtype(kdt))
        kmiss = np.zeros(max(n, 1), np.uint8) if kdt & ir.NULLABLE else None
        out.data = karr.ctypes.data
        if kmiss is not None:
            out.missing = kmiss.ctypes.data
    counts = np.zeros(max(n, 1), np.int64); vi = np.zeros(max(n, 1), np.int64); vf = np.zeros(max(n, 1), np.float64)
    N.check(L.dfdb_query_groupreduce_fetch(q._h, C.byref(out), counts.ctypes.data, vi.ctypes.data, vf.ctypes.data))
    if (kdt & ir.DTYPE_MASK) == ir.STRING:
        keys = _to_user((ksz[:n].copy(), kby[:out.nbytes].copy()))
    elif kdt & ir.NULLABLE:
        keys = np.ma.masked_array(karr[:n].copy(), mask=kmiss[:n].astype(bool))
    else:
        keys = karr[:n].copy()
    return keys, counts[:n].copy(), vi[:n].copy(), vf[:n].copy(), (q.coltype(1) & ir.DTYPE_MASK if with_value else None)


def _groupreduce_frame(by: str, stat: str, keys, counts, vi, vf, vdt):
    import pandas as pd
    res = {by: keys, "count": counts}
    if stat != "count":
        isf = vdt in (ir.F32, ir.F64)
        uns = vdt in (ir.U8, ir.U16, ir.U32, ir.U64)
        vals = vf if isf else (vi.astype(np.uint64) if uns and stat != "mean" else vi)
        if stat == "mean":
            vals = (vf if isf else (vi.astype(np.uint64).astype(np.float64) if uns else vi.astype(np.float64))) / np.maximum(counts, 1)
        res[stat] = vals
    return pd.DataFrame(res)


def _key_out(kdt: int, n: int, kb: int):
    """a host dfdb_outcol for n keys of dtype kdt (kb string bytes) -> (outcol, a function that returns the keys as _groupreduce_raw does)"""
    out = N.OutCol()
    out.memkind = N.MEM_HOST
    if (kdt & ir.DTYPE_MASK) == ir.STRING:
        ksz = np.empty(max(n, 1), np.int32); kby = np.empty(max(kb, 1), np.uint8)
        out.data, out.bytes, out.bytes_cap = ksz.ctypes.data, kby.ctypes.data, kb
        return out, lambda: _to_user((ksz[:n].copy(), kby[:out.nbytes].copy()))
    karr = np.empty(max(n, 1), ir.numpy_of_dtype(kdt))
    kmiss = np.zeros(max(n, 1), np.uint8) if kdt & ir.NULLABLE else None
    out.data = karr.ctypes.data
    if kmiss is not None:
        out.missing = kmiss.ctypes.data
        return out, lambda: np.ma.masked_array(karr[:n].copy(), mask=kmiss[:n].astype(bool))
    return out, lambda: karr[:n].copy()


def _groupreduce_n_raw(q: "_Query", nkeys: int, vidx, stats):
    """dfdb_query_groupreduce_n + _fetch: keys are projection columns [0, nkeys), reducer i is stats[i] over projection column vidx[i] ->
    (list of key arrays, counts, values as Int64 bits [nvals, ng], values as Float64 [nvals, ng])"""
    L = N.load()
    nv = len(stats)
    kc = (C.c_int32 * nkeys)(*range(nkeys))
    vc = (C.c_int32 * max(nv, 1))(*vidx)
    st = (C.c_int32 * max(nv, 1))(*[_STATS[s] for s in stats])
    ng, kb = C.c_int64(), (C.c_int64 * nkeys)()
    N.check(L.dfdb_query_groupreduce_n(q._h, kc, nkeys, vc, st, nv, C.byref(ng), kb))
    n = ng.value
    outs = (N.OutCol * nkeys)()
    getters = []
    for k in range(nkeys):
        o, get = _key_out(q.coltype(k), n, kb[k])
        outs[k] = o
        getters.append((o, get))
    counts = np.zeros(max(n, 1), np.int64); vi = np.zeros(max(n * nv, 1), np.int64); vf = np.zeros(max(n * nv, 1), np.float64)
    N.check(L.dfdb_query_groupreduce_n_fetch(q._h, outs, counts.ctypes.data, vi.ctypes.data, vf.ctypes.data))
    for k in range(nkeys):
        getters[k][0].nbytes = outs[k].nbytes
    keys = [get() for _, get in getters]
    return keys, counts[:n].copy(), vi[:n * nv].reshape(nv, n).copy(), vf[:n * nv].reshape(nv, n).copy()


def _groupreduce_n(v: Union[DFView, DFTable], by, reducers: dict):
    import pandas as pd
    v = v if isinstance(v, DFView) else DFView(v)
    by = list(by)
    if not 1 <= len(by) <= 8:
        raise ValueError(f"ArgumentError: groupreduce takes 1 to 8 key columns, not {len(by)}")
    if len(set(by)) != len(by):
        raise ValueError("ArgumentError: a key column appears twice in `by`")
    names = list(by)
    specs = []
    for name, spec in reducers.items():
        if name in by or name == "count":
            raise ValueError(f"ArgumentError: the result column {name!r} would be named twice")
        if not (isinstance(spec, (tuple, list)) and len(spec) == 2):
            raise ValueError(f"ArgumentError: reducer {name!r} must be (column, stat)")
        c, stat = spec
        if stat not in _STATS:
            raise ValueError(f"ArgumentError: unknown statistic {stat}")
        if stat != "count" and c not in names:
            names.append(c)
        specs.append((name, c, stat))
    if len(specs) > 16:
        raise ValueError(f"ArgumentError: groupreduce takes 0 to 16 reducers, not {len(specs)}")
    sub = DFView(v.table, Projection({nm: v.projection.cols[nm] for nm in names}), v.selection)
    q = _Query(sub)
    vidx = [names.index(c) if stat != "count" else -1 for _, c, stat in specs]
    keys, counts, vi, vf = _groupreduce_n_raw(q, len(by), vidx, [stat for _, _, stat in specs])
    res = {b: k for b, k in zip(by, keys)}
    res["count"] = counts
    for i, (name, c, stat) in enumerate(specs):
        if stat == "count":
            res[name] = counts
            continue
        vdt = q.coltype(vidx[i]) & ir.DTYPE_MASK
        isf = vdt in (ir.F32, ir.F64)
        uns = vdt in (ir.U8, ir.U16, ir.U32, ir.U64)
        vals = vf[i] if isf else (vi[i].astype(np.uint64) if uns and stat != "mean" else vi[i])
        if stat == "mean":
            vals = (vf[i] if isf else (vi[i].astype(np.uint64).astype(np.float64) if uns else vi[i].astype(np.float64))) / np.maximum(counts, 1)
        res[name] = vals
    return pd.DataFrame(res)


def groupreduce(v: Union[DFView, DFTable], by, col: Optional[str] = None, stat: str = "count", **reducers):
    """groupreduce(view, (:by,); out = :col => Stat()): one row per distinct value of `by` over the view's selected rows, in order of first
    appearance (the reference's group_map numbering), with the group's row count and stat(col) — stat in count / sum / min / max / mean.
    Returns a pandas.DataFrame with columns [by, "count", stat].

    groupreduce(view, ("a", "b"), name=("col", "stat"), ...) (aggregate.jl:1-14: a tuple of keys, any number of `name = col => Stat()`): one row per
    distinct tuple, in order of the first selected row that holds it, with the count and every reducer — one device pass for all of them
    (dfdb_query_groupreduce_n).  Columns [*by, "count", *names] in keyword order.  A tuple `by` with col / stat alone is one reducer named stat."""
    if isinstance(by, str) and not reducers:
        sub, with_value = _groupreduce_view(v, by, col, stat)
        return _groupreduce_frame(by, stat, *_groupreduce_raw(_Query(sub), with_value, stat))
    if reducers and (col is not None or stat != "count"):
        raise ValueError("ArgumentError: give either col / stat or name=(col, stat) reducers, not both")
    if isinstance(by, str):
        by = (by,)
    elif not isinstance(by, (tuple, list)):
        raise ValueError(f"ArgumentError: `by` must be a column name or a tuple of them, not {type(by).__name__}")
    if not reducers and (col is not None or stat != "count"):
        reducers = {stat: (col, stat)}
    return _groupreduce_n(v, by, reducers)
