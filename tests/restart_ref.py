"""The header of a POP 'bin' restart file, restated in plain Python from the reference's io_binary.F90 and restart.F90 -- not from this
library's host_restart.cpp, which it is there to check.  No GPU, no package import.

write_header   the file open_binary (io_binary.F90:413-560) and define_field_binary (:795-934) write, for a list of attributes in the
               order restart.F90 adds them (reference_globals) and a list of fields
read_header    the file as open_read_binary (:219-312) and define_field_binary (:976-1111) read it: what the reference would make of a
               header, whoever wrote it, and what it would stop at

The format.  Text, one item per line.  "&GLOBAL", then "name:type:value" lines: title, history, a conventions line whose name is
damaged (see CONVENTIONS_NAME), then the attributes grouped by type -- char, log, int, r4, r8 -- each group in the order the attributes
were added.  Every one of these lines is written with an (a80) edit descriptor: blank-padded to 80 columns, and cut there.  Then one
section per field: "&SHORT_NAME", long_name, units, grid_loc (each only if set; plain text after the second separator), "id:int:<first
record>", "nfield_dims:int:<2|3>", "/"; these lines are trimmed.  open_binary writes no "/" after the global attributes (end_global=False
reproduces that); the reader then takes the first field section for attributes too, harmlessly, and stops at its "/".

Values are list-directed output, whose layout the compiler chooses.  Two styles are written here:
  gfortran   a leading blank; integers right-justified in 11 columns; T / F; reals as G25.17E3 (r8) and G16.9E2 (r4) lay them out
             ("   3600.0000000000000     "): 17 significant digits, so that an r8 survives the round trip bit for bit
  compact    no blanks at all; integers as they are; reals with an E exponent ("3.6000000000000000E+03")
"""
import math
import re

SEP = ":"                                   # attrib_separator, io_binary.F90:59
LINE = 80                                   # (a80)
TYPES = ("char", "log", "int", "r4", "r8")  # the order of the groups open_binary writes
# work_line(1:11) = 'conventions', then work_line(11:14) = 'char' lands on the last letter of the name and on the separator
# (io_binary.F90:435-441): the line has one separator, and no reader can tell its name from its type
CONVENTIONS_NAME = "conventiochar"
_TYPE_NAMES = {            # open_read_binary :293-309; the field sections also take 'character' and 'integer' (:1079-1102)
    "char": ("char", "CHAR"), "log": ("log", "LOG", "logical", "LOGICAL"), "int": ("int", "INT", "i4", "I4"),
    "r4": ("r4", "R4", "REAL", "real", "float", "FLOAT"), "r8": ("r8", "R8", "dbl", "DBL", "double", "DOUBLE")}
_FIELD_TYPE_NAMES = dict(_TYPE_NAMES, char=_TYPE_NAMES["char"] + ("character", "CHARACTER"), int=_TYPE_NAMES["int"] + ("integer", "INTEGER"))

# the attributes of write_restart, restart.F90:1281-1348, in the order of the calls, with the type of the variable each one passes
_REFERENCE_GLOBALS = [
    ("runid", "char"), ("iyear", "int"), ("imonth", "int"), ("iday", "int"), ("ihour", "int"), ("iminute", "int"), ("isecond", "int"),
    ("iyear0", "int"), ("imonth0", "int"), ("iday0", "int"), ("ihour0", "int"), ("iminute0", "int"), ("isecond0", "int"), ("dtt", "r8"),
    ("iday_of_year", "int"), ("iday_of_year_last", "int"), ("elapsed_days", "int"), ("elapsed_months", "int"), ("elapsed_years", "int"),
    ("elapsed_days_this_year", "int"), ("seconds_this_day", "r8"), ("seconds_this_day_next", "r8"), ("seconds_this_year", "r8"),
    ("seconds_this_year_next", "r8"), ("nsteps_total", "int"), ("eod", "log"), ("eod_last", "log"), ("eom", "log"), ("eom_last", "log"),
    ("eom_next", "log"), ("eoy", "log"), ("eoy_last", "log"), ("midnight_last", "log"), ("adjust_year_next", "log"), ("newday", "log"),
    ("newhour", "log"), ("leapyear", "log"), ("days_in_year", "int"), ("days_in_prior_year", "int"), ("seconds_in_year", "r8"),
    ("hours_in_year", "r8"), ("tlast_ice", "r8"), ("lcoupled_ts", "log"), ("shf_interp_last", "r8"), ("sfwf_interp_last", "r8"),
    ("ws_interp_last", "r8"), ("ap_interp_last", "r8"), ("pt_interior_interp_last", "r8"), ("s_interior_interp_last", "r8"),
    ("sum_precip", "r8"), ("precip_fact", "r8"), ("ssh_initial", "r8")]
REFERENCE_NAMES = frozenset(n for n, _ in _REFERENCE_GLOBALS) | {"title", "history", "conventions"}
_MONTH_DAYS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)


def is_reference_name(name):
    """an attribute write_restart writes: the fixed list, sal_initialNNN (:1372-1376), rf_S_prev_<tracer> and rf_Svol_prev_<tracer>
    (:1356-1370)"""
    return (name in REFERENCE_NAMES or re.fullmatch(r"sal_initial\d{3}", name) is not None
            or re.fullmatch(r"rf_S(vol)?_prev_\w+", name) is not None)


def reference_globals(nsteps_total, eod, eod_last, tlast_ice, lcoupled_ts, dtt, km, robert=None, sal_initial=None, runid="restart_ref"):
    """Every attribute of restart.F90:1281-1376 as (name, type, value), in the order write_restart adds them, for a run that began at
    0001-01-01 00:00 with 365-day years and has taken nsteps_total steps of dtt seconds.  robert: None, or a list of
    (tracer short name, rf_S_prev, rf_Svol_prev) -- first every rf_S_prev_<name>, then every rf_Svol_prev_<name>.  sal_initial: km
    values (default 0.035 g/g at every level)."""
    secs = nsteps_total * dtt
    day = int(secs // 86400.0)
    sod = secs - 86400.0 * day
    doy = day % 365
    month, dom = 1, doy
    while dom >= _MONTH_DAYS[month - 1]:
        dom -= _MONTH_DAYS[month - 1]; month += 1
    soy = 86400.0 * doy + sod
    never = 1.0e20                             # what the forcing modules hold in *_interp_last when they never interpolate
    v = dict(runid=runid, iyear=1 + day // 365, imonth=month, iday=dom + 1, ihour=int(sod) // 3600, iminute=int(sod) % 3600 // 60,
             isecond=int(sod) % 60, iyear0=1, imonth0=1, iday0=1, ihour0=0, iminute0=0, isecond0=0, dtt=dtt, iday_of_year=doy + 1,
             iday_of_year_last=doy + 1, elapsed_days=day, elapsed_months=12 * (day // 365) + month - 1, elapsed_years=day // 365,
             elapsed_days_this_year=doy, seconds_this_day=sod, seconds_this_day_next=sod + dtt, seconds_this_year=soy,
             seconds_this_year_next=soy + dtt, nsteps_total=nsteps_total, eod=bool(eod), eod_last=bool(eod_last), eom=False, eom_last=False,
             eom_next=False, eoy=False, eoy_last=False, midnight_last=bool(eod_last), adjust_year_next=False, newday=bool(eod_last),
             newhour=False, leapyear=False, days_in_year=365, days_in_prior_year=365, seconds_in_year=365 * 86400.0, hours_in_year=8760.0,
             tlast_ice=tlast_ice, lcoupled_ts=bool(lcoupled_ts), shf_interp_last=never, sfwf_interp_last=never, ws_interp_last=never,
             ap_interp_last=never, pt_interior_interp_last=never, s_interior_interp_last=never, sum_precip=0.0, precip_fact=1.0,
             ssh_initial=0.0)
    out = [(n, t, v[n]) for n, t in _REFERENCE_GLOBALS]
    if robert:
        out += [("rf_S_prev_" + n, "r8", s) for n, s, _ in robert]
        out += [("rf_Svol_prev_" + n, "r8", sv) for n, _, sv in robert]
    sal = [0.035] * km if sal_initial is None else list(sal_initial)
    assert len(sal) == km
    out += [("sal_initial%03d" % (k + 1), "r8", sal[k]) for k in range(km)]
    return out


# ---- list-directed output ---------------------------------------------------------------------------------------------------------
def _g_real(x, w, sig, expw):
    """Gw.(sig)E(expw) of a real: sig significant digits, fixed-point when the exponent allows (then expw + 2 trailing blanks)"""
    tail = expw + 2
    mant, e = ("%.*e" % (sig - 1, x)).split("e")
    e = int(e)
    if x == 0.0 or -1 <= e < sig:
        return ("%.*f" % (sig - 1 - (e if x != 0.0 else 0), x)).rjust(w - tail) + " " * tail
    return ("%sE%s%0*d" % (mant, "-" if e < 0 else "+", expw, abs(e))).rjust(w)


def format_value(typ, value, style="gfortran"):
    """the text write(line(n:),*) value leaves, in the given style"""
    if style not in ("gfortran", "compact"):
        raise ValueError("unknown style " + style)
    lead = " " if style == "gfortran" else ""
    if typ == "char":
        return lead + str(value)
    if typ == "log":
        return lead + ("T" if value else "F")
    if typ == "int":
        return lead + ("%11d" if style == "gfortran" else "%d") % int(value)
    if typ in ("r4", "r8"):
        if not math.isfinite(value):
            raise ValueError("no list-directed form restated for %r" % value)
        if style == "gfortran":
            return lead + (_g_real(value, 25, 17, 3) if typ == "r8" else _g_real(value, 16, 9, 2))
        return ("%.16E" if typ == "r8" else "%.8E") % value
    raise ValueError("unknown attribute type " + typ)


def write_header(path, attrs, fields, style="gfortran", title="POP restart", history="restart_ref.write_header", conventions="POP restart",
                 end_global=True):
    """<path>.hdr.  attrs: (name, type, value) in the order of the add_attrib_file calls (they are written grouped by type).  fields:
    dicts with name, id, ndims and optionally long_name, units, grid_loc, in file order.  end_global: put "/" after the global
    attributes (open_binary itself does not)."""
    def a80(s):
        return "%-80s" % s[:LINE]
    out = [a80("&GLOBAL"),
           a80("title" + SEP + "char" + SEP + format_value("char", title, style)),
           a80("history" + SEP + "char" + SEP + format_value("char", history, style)),
           a80(CONVENTIONS_NAME + SEP + format_value("char", conventions, style))]
    for typ in TYPES:
        for name, t, value in attrs:
            if t not in TYPES:
                raise ValueError("unknown attribute type %s of %s" % (t, name))
            if t == typ:
                out.append(a80(name + SEP + t + SEP + format_value(t, value, style)))
    if end_global:
        out.append(a80("/"))
    for f in fields:
        out.append("&" + f["name"])
        for key in ("long_name", "units", "grid_loc"):
            if f.get(key):
                out.append(key + SEP + "char" + SEP + f[key])
        out.append(("id" + SEP + "int" + SEP + format_value("int", f["id"], style)).rstrip())
        out.append(("nfield_dims" + SEP + "int" + SEP + format_value("int", f["ndims"], style)).rstrip())
        out.append("/")
    with open(path + ".hdr", "w") as h:
        h.write("".join(ln + "\n" for ln in out))


# ---- list-directed input ----------------------------------------------------------------------------------------------------------
class HeaderError(Exception):
    """the reference would stop here"""


def _first_item(text, what):
    t = text.lstrip(" \t")
    m = re.match(r"[^ \t,/]+", t)
    if not m:
        raise HeaderError("no value to read for %s in %r" % (what, text))      # end of record, or a null value
    return m.group(0)


def parse_value(typ, text, what=""):
    """read(text,*) into a variable of the given type: the first item of the record; blanks, a comma or a slash end it"""
    if typ == "char":
        return text.rstrip()                       # trim(work_line): not a list-directed read
    item = _first_item(text, what)
    if typ == "log":
        m = re.match(r"\.?([TtFf])", item)         # an optional period, T or F, then anything
        if not m:
            raise HeaderError("not a logical for %s: %r" % (what, text))
        return m.group(1) in "Tt"
    if typ == "int":
        if not re.fullmatch(r"[+-]?\d+", item):
            raise HeaderError("not an integer for %s: %r" % (what, text))
        return int(item)
    if typ in ("r4", "r8"):
        m = re.fullmatch(r"([+-]?(?:\d+\.?\d*|\.\d+))(?:[EeDdQq]([+-]?\d+)|([+-]\d+))?", item)
        if not m:
            raise HeaderError("not a real for %s: %r" % (what, text))
        return float(m.group(1) + "e" + (m.group(2) or m.group(3) or "0"))
    raise ValueError(typ)


def _split(line):
    """name, type, value of one line as both readers take it apart (:253-275, :1015-1039): the name is what stands before the first
    separator, the type what stands before the next one once the line has been shifted left, the value the rest, shifted left again.
    A separator that is not there gives an empty name or type and leaves the line as it is."""
    i = line.find(SEP)
    name = line[:i] if i >= 0 else ""
    rest = (line[i + 1:] if i >= 0 else line).lstrip(" ")
    j = rest.find(SEP)
    typ = rest[:j] if j >= 0 else ""
    value = (rest[j + 1:] if j >= 0 else rest).lstrip(" ")
    return name.rstrip(), typ.rstrip(), value.rstrip()


def _canonical(typ, table):
    for t, names in table.items():
        if typ in names:
            return t
    return None


class Header:
    """What the reference holds after open_read_binary: title, history, conventions; attrs: name -> (type, value), a later line of the
    same name replacing an earlier one; ignored: lines of the global section that add nothing (no or unknown type).  problems: what it
    would have stopped at.  too_long: numbers (1-based) of the lines it saw cut at 80 columns."""

    def __init__(self, lines):
        self.lines, self.title, self.history, self.conventions = lines, None, None, None
        self.attrs, self.ignored, self.problems, self.too_long = {}, [], [], []

    def find_section(self, name):
        """define_field_binary :978-989: index of the first line, from the top, that begins with '&' + name; HeaderError if none"""
        want = "&" + name.rstrip()
        for n, ln in enumerate(self.lines):
            if ln.startswith(want):
                return n
        raise HeaderError("could not find field in binary header file: " + name)

    def field(self, name):
        """the io field the reference defines from the section of `name` (:996-1114): section (the name on the line found), id,
        nfield_dims, long_name, units, grid_loc, coordinates, and any further attribute; HeaderError where it would abort"""
        n = self.find_section(name)
        out = {"section": self.lines[n][1:].rstrip()}
        for ln in self.lines[n + 1:]:
            if ln[:1] == "/":
                return out
            aname, typ, value = _split(ln)
            key = aname.lower() if aname in ("long_name", "LONG_NAME", "units", "UNITS", "coordinates", "COORDINATES", "grid_loc", "GRID_LOC",
                                              "id", "ID", "nfield_dims", "NFIELD_DIMS", "valid_range", "VALID_RANGE", "field_dim", "FIELD_DIM") else None
            what = "%s of %s" % (aname, name)
            if key in ("long_name", "units", "coordinates", "grid_loc"):
                out[key] = value
            elif key in ("id", "nfield_dims"):
                out[key] = parse_value("int", value, what)
            elif key == "valid_range":
                out[key] = parse_value("r8", value, what)
            elif key == "field_dim":
                pass
            else:
                t = _canonical(typ, _FIELD_TYPE_NAMES)
                if t is None:
                    raise HeaderError("define_io_field: unknown data type %r (%s)" % (typ, what))
                out[aname] = parse_value(t, value, what)
        raise HeaderError("define_io_field: error reading attribute from header (no '/' ends the section of %s)" % name)


def read_header(path, fields=()):
    """<path>.hdr under the reference's rules.  Returns a Header; with `fields`, .fields maps each name to Header.field(name), and a
    field the reference would abort on is listed in .problems instead."""
    with open(path + ".hdr") as h:
        raw = h.read().split("\n")
    if raw and raw[-1] == "":
        raw.pop()
    hd = Header([ln[:LINE].lstrip(" ") for ln in raw])        # read '(a80)', then adjustl
    hd.too_long = [n + 1 for n, ln in enumerate(raw) if len(ln.rstrip(" ")) > LINE]
    n = 0
    while n < len(hd.lines) and hd.lines[n][:7] != "&GLOBAL":
        n += 1
    if n == len(hd.lines):
        hd.problems.append("no &GLOBAL section")
    for ln in hd.lines[n + 1:]:                               # the end of the file ends the loop as "/" does
        if ln[:1] == "/":
            break
        name, typ, value = _split(ln)
        if name in ("title", "TITLE"):
            hd.title = value
        elif name in ("history", "HISTORY"):
            hd.history = value
        elif name in ("conventions", "CONVENTIONS"):
            hd.conventions = value
        else:
            t = _canonical(typ, _TYPE_NAMES)
            if t is None:
                hd.ignored.append(ln.rstrip())                # select case without a default: nothing happens
                continue
            try:
                hd.attrs[name] = (t, parse_value(t, value, name))
            except HeaderError as e:
                hd.problems.append(str(e))
    hd.fields = {}
    for f in fields:
        try:
            hd.fields[f] = hd.field(f)
        except HeaderError as e:
            hd.problems.append(str(e))
    return hd


def parse_hdr(path):
    """<path>.hdr read plainly, without the reference's rules: section -> {name: (type text, value text)}"""
    sec, cur = {}, None
    for line in open(path + ".hdr"):
        line = line.strip()
        if line.startswith("&"):
            cur = line[1:].strip(); sec[cur] = {}
        elif line.startswith("/"):
            cur = None
        elif cur is not None and line.count(":") >= 2:
            name, typ, val = line.split(":", 2)
            sec[cur][name.strip()] = (typ.strip(), val.strip())
    return sec
