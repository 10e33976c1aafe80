"""What the String x String comparison tests share: the four-line definition on `bytes`, the content table, and StrPair, which holds one table twice
(oracle + engine) as helpers.Pair does, with bytes values and an explicit Union{String,Missing} dtype per column."""


def cmp(a: bytes, b: bytes) -> int:
    """Base.cmp(::String, ::String): memcmp over the common prefix, then the lengths, bytes unsigned — Python orders `bytes` the same way"""
    return (a > b) - (a < b)


OPS = {"==": lambda c: c == 0, "!=": lambda c: c != 0, "<": lambda c: c < 0, "<=": lambda c: c <= 0, ">": lambda c: c > 0, ">=": lambda c: c >= 0}
IR_OPS = {"==": lambda p, q: p == q, "!=": lambda p, q: p != q, "<": lambda p, q: p < q, "<=": lambda p, q: p <= q, ">": lambda p, q: p > q, ">=": lambda p, q: p >= q}


def expect(op, a, b):
    """one row of `a OP b`: True / False, None where either side is missing"""
    return None if a is None or b is None else bool(OPS[op](cmp(a, b)))


def content_pairs():
    P = [(b"", b""), (b"", b"a")]
    for n in (7, 8, 9, 15, 16, 17, 64):
        s = bytes(65 + i % 26 for i in range(n))
        P += [(s, s), (s, s[:-1] + b"~"), (s[:-1] + b"!", s), (s, s[:n // 2]), (s[:n // 2], s)]      # equal; last byte differs, both ways; a proper prefix, both ways
    P += [("ÿ".encode(), b"\x7f"), (b"\x7f", "ÿ".encode()),                                          # bytes >= 0x80 against bytes < 0x80: a signed compare fails
          (b"a\0b", b"a\0c"), (b"a\0c", b"a\0b"), (b"a\0", b"a"),                                    # embedded NUL
          (b"abcd", b"abce"), (b"abcdefgh1", b"abcdefgh2"),                                          # equal sizes, unequal bytes
          (b"abc", b"abcdef"), (b"abcx", b"abcdefgh"),                                               # unequal sizes, a shared prefix
          (b"x" * 199 + b"a", b"x" * 199 + b"b"), (b"x" * 199 + b"b", b"x" * 199 + b"a"), (b"x" * 200, b"x" * 200)]
    return P


FILL = [(b"ab", b"ab"), (b"abc", b"abd"), (b"", b"q"), (b"zz", b"z"), (b"k\xc3", b"k\x7f"), (b"same", b"same"), (b"a", b"b")]


def content_columns(n, lean=False):
    """the content table repeated to n rows from an offset that is no multiple of 64.  lean: fifteen short filler pairs after every content pair — mostly
    short strings with a long one now and then, the shape of real columns (the content table alone is ~37 bytes a row)"""
    P = content_pairs()
    if not lean:
        rows = [P[(i + 5) % len(P)] for i in range(n)]
    else:
        rows = [P[((i // 16) + 5) % len(P)] if i % 16 == 3 else FILL[(i * 5 + i // 16) % len(FILL)] for i in range(n)]
    return [r[0] for r in rows], [r[1] for r in rows]


class S:
    """a String column: values are bytes / None; nullable makes the dtype Union{String,Missing} whether or not a row is missing"""

    def __init__(self, values, nullable=False):
        self.values, self.nullable = list(values), nullable or any(v is None for v in values)


class StrPair:
    """what helpers.apply_stages and helpers.assert_same read of a helpers.Pair (O, dfdb, names, nrows, o, d), over `cols`: name -> S or numpy array"""

    def __init__(self, O, dfdb, cols, block_size=65536, via_files=None, ctx=None):
        from dfdb import ir
        self.O, self.dfdb, self.names = O, dfdb, list(cols)
        first = next(iter(cols.values()))
        self.nrows = len(first.values if isinstance(first, S) else first)
        self.o = O.Table(block_size=block_size)
        for k, v in cols.items():
            if isinstance(v, S):
                self.o.add_column(k, O.strings_to_flat(v.values), dtype=O.NULLABLE if v.nullable else None)
            else:
                self.o.add_column(k, v)
        if via_files:
            self.o.save(via_files)
            self.d = dfdb.open_table(via_files, ctx=ctx) if ctx is not None else dfdb.open_table(via_files)
        else:
            self.d = dfdb.DFTable.new(block_size, ctx)
            for k, v in cols.items():
                if isinstance(v, S):
                    self.d.add_column(k, v.values, dtype=ir.STRING | (ir.NULLABLE if v.nullable else 0))
                else:
                    self.d.add_column(k, v)


def build(O, dfdb, cols, block_size=65536, via_files=None, ctx=None):
    return StrPair(O, dfdb, cols, block_size, via_files, ctx)
