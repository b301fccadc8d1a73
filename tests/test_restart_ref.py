"""tests/restart_ref.py against itself and against the rules of the reference's header reader (io_binary.F90:219-312, 976-1111):
what the GPU restart tests lean on.  No GPU."""
import struct

import pytest

import restart_ref as rr

KM = 5
FIELDS = [dict(name="UBTROP_CUR", id=1, ndims=2, long_name="U barotropic velocity at current time", units="cm/s", grid_loc="2220"),
          dict(name="FW_OLD", id=2, ndims=2, long_name="fresh water input at old time", grid_loc="2110"),
          dict(name="TEMP_CUR", id=3, ndims=3, long_name="Potential temperature at current time", units="degC", grid_loc="3111"),
          dict(name="TEMP_OLD", id=3 + KM, ndims=3)]
# values whose decimal form needs all 17 digits, a power of two, one below 0.1, one past 1e17, zero and a negative one
R8 = [3600.0, 0.1, 1.0 / 3.0, 2.0 ** -40, 0.034999999999999996, 1.0e20, 0.0, -86400.5, 123456789012345678.0, 5e-324, 1.7976931348623157e308]


def globals_(**kw):
    a = dict(nsteps_total=123, eod=True, eod_last=False, tlast_ice=5400.0, lcoupled_ts=False, dtt=3600.0, km=KM,
             robert=[("TEMP", 1.0 / 3.0, -2.5e-7), ("SALT", 0.1, 7.0e22)], sal_initial=[0.03 + 1e-3 / (k + 3) for k in range(KM)])
    a.update(kw)
    return rr.reference_globals(**a)


@pytest.mark.parametrize("end_global", [True, False])
@pytest.mark.parametrize("style", ["gfortran", "compact"])
def test_write_then_read_is_the_identity(tmp_path, style, end_global):
    attrs = globals_() + [("probe%02d" % i, "r8", v) for i, v in enumerate(R8)] + [("single", "r4", 0.15625), ("big", "int", -2147483647)]
    path = str(tmp_path / "r.bin")
    rr.write_header(path, attrs, FIELDS, style=style, title="a title", history="a history: with a colon", end_global=end_global)
    hd = rr.read_header(path, fields=[f["name"] for f in FIELDS])
    assert hd.problems == [] and hd.too_long == []
    assert hd.title == "a title" and hd.history == "a history: with a colon" and hd.conventions is None
    # every attribute with its type and its value, reals bit for bit
    want = {n: (t, v) for n, t, v in attrs}
    got = dict(hd.attrs)
    if not end_global:          # open_binary's own file: the first field's section is read as attributes too, up to its "/"
        assert got.pop("long_name") == ("char", FIELDS[0]["long_name"]) and got.pop("units") == ("char", "cm/s")
        assert got.pop("grid_loc") == ("char", "2220") and got.pop("id") == ("int", 1) and got.pop("nfield_dims") == ("int", 2)
        assert "&UBTROP_CUR" in hd.ignored
    assert set(got) == set(want)
    for n, (t, v) in want.items():
        assert got[n][0] == t, n
        if t == "r8":
            assert struct.pack("<d", got[n][1]) == struct.pack("<d", v), (n, v, got[n][1])
        else:
            assert got[n][1] == v and type(got[n][1]) is type(v), n
    for f in FIELDS:
        g = hd.fields[f["name"]]
        assert g["section"] == f["name"] and g["id"] == f["id"] and g["nfield_dims"] == f["ndims"]
        for key in ("long_name", "units", "grid_loc"):
            assert g.get(key) == f.get(key), (f["name"], key)


def test_layout_is_the_reference_s(tmp_path):
    """&GLOBAL, title, history, the damaged conventions line, then char, log, int, r4, r8 in the order added; global lines 80 columns
    wide; field lines trimmed; the two value styles"""
    path = str(tmp_path / "r.bin")
    attrs = globals_() + [("single", "r4", 0.5)]
    rr.write_header(path, attrs, FIELDS)
    lines = open(path + ".hdr").read().split("\n")
    assert lines.pop() == ""
    end = lines.index("/".ljust(80))
    assert all(len(ln) == 80 for ln in lines[:end + 1]) and all(ln == ln.rstrip() and len(ln) < 80 for ln in lines[end + 1:])
    assert [ln.rstrip() for ln in lines[:5]] == ["&GLOBAL", "title:char: POP restart", "history:char: restart_ref.write_header",
                                                 "conventiochar: POP restart", "runid:char: restart_ref"]
    types = [ln.split(":")[1] for ln in lines[4:end]]
    assert types == sorted(types, key=rr.TYPES.index) and set(types) == set(rr.TYPES)
    for typ in rr.TYPES:
        assert [ln.split(":")[0] for ln in lines[4:end] if ln.split(":")[1] == typ] == [n for n, t, _ in attrs if t == typ]
    names = [n for n, _, _ in attrs]
    assert names[:3] == ["runid", "iyear", "imonth"] and names.index("eod") + 1 == names.index("eod_last") == names.index("nsteps_total") + 2
    assert names.index("tlast_ice") + 1 == names.index("lcoupled_ts")
    assert names[-KM - 5:-1] == ["rf_S_prev_TEMP", "rf_S_prev_SALT", "rf_Svol_prev_TEMP", "rf_Svol_prev_SALT"] + ["sal_initial%03d" % k for k in range(1, KM + 1)]
    assert "nsteps_total:int:         123".ljust(80) in lines and "eod:log: T".ljust(80) in lines and "eod_last:log: F".ljust(80) in lines
    assert "dtt:r8:   3600.0000000000000     ".ljust(80) in lines and "precip_fact:r8:   1.0000000000000000     ".ljust(80) in lines
    assert "shf_interp_last:r8:   1.0000000000000000E+020".ljust(80) in lines and "single:r4:  0.500000000    ".ljust(80) in lines
    k = lines.index("&TEMP_CUR")
    assert lines[k:k + 7] == ["&TEMP_CUR", "long_name:char:Potential temperature at current time", "units:char:degC", "grid_loc:char:3111",
                              "id:int:           3", "nfield_dims:int:           3", "/"]
    rr.write_header(path, attrs, FIELDS, style="compact")
    text = open(path + ".hdr").read().split("\n")
    assert "nsteps_total:int:123".ljust(80) in text and "eod:log:T".ljust(80) in text and "dtt:r8:3.6000000000000000E+03".ljust(80) in text
    assert "id:int:3" in text and "title:char:POP restart".ljust(80) in text


def test_a_line_longer_than_80_columns_is_seen_truncated(tmp_path):
    path = str(tmp_path / "r.bin")
    with open(path + ".hdr", "w") as h:
        h.write("&GLOBAL\n")
        h.write("runid:char:" + "x" * 100 + "\n")                                 # cut inside the value
        h.write("%s:int: 12345\n" % ("n" * 70))                                    # the value loses its last digits
        h.write("%s:int: 7\n" % ("m" * 74))                                        # nothing of the value is left: the read fails
        h.write("/\n&PSURF_CUR\n")
        h.write("long_name:char:" + "y" * 90 + "\nid:int:" + " " * 70 + "123456\n/\n")
    hd = rr.read_header(path, fields=["PSURF_CUR"])
    assert hd.too_long == [2, 3, 4, 7, 8]
    assert hd.attrs["runid"] == ("char", "x" * 69) and hd.attrs["n" * 70] == ("int", 1234)
    assert "m" * 74 not in hd.attrs and len(hd.problems) == 1 and "m" * 74 in hd.problems[0]
    assert hd.fields["PSURF_CUR"]["long_name"] == "y" * 65 and hd.fields["PSURF_CUR"]["id"] == 123
    # the writer cuts its own global lines the same way
    rr.write_header(path, [("runid", "char", "z" * 100)], [], title="t" * 100)
    hd = rr.read_header(path)
    assert hd.too_long == [] and hd.title == "t" * 68 and hd.attrs["runid"] == ("char", "z" * 68)


def test_the_prefix_rule_finds_the_first_match(tmp_path):
    path = str(tmp_path / "r.bin")
    fields = [dict(name="TEMP_CURRENT", id=40, ndims=3), dict(name="TEMP_CUR", id=3, ndims=3), dict(name="IAGE_3_CUR", id=50, ndims=3),
              dict(name="IAGE_CUR", id=60, ndims=3), dict(name="TEMP_CUR", id=99, ndims=3)]
    rr.write_header(path, globals_(), fields)
    hd = rr.read_header(path, fields=["TEMP_CUR", "IAGE_CUR", "IAGE", "TEMP_CURRENT", "SALT_CUR", "GLOB"])
    assert hd.fields["TEMP_CUR"]["section"] == "TEMP_CURRENT" and hd.fields["TEMP_CUR"]["id"] == 40
    assert hd.fields["TEMP_CURRENT"]["id"] == 40
    assert hd.fields["IAGE_CUR"]["section"] == "IAGE_CUR" and hd.fields["IAGE_CUR"]["id"] == 60      # "&IAGE_3_CUR" does not begin with "&IAGE_CUR"
    assert hd.fields["IAGE"]["section"] == "IAGE_3_CUR"
    assert "SALT_CUR" not in hd.fields and "GLOB" not in hd.fields
    # SALT_CUR is not there; "&GLOBAL" begins with "&GLOB", and its attribute lines are then read as a field's: runid has a type the
    # field reader knows, the damaged conventions line has none
    assert len(hd.problems) == 2 and "could not find field" in hd.problems[0] and "SALT_CUR" in hd.problems[0]
    assert "unknown data type" in hd.problems[1] and rr.CONVENTIONS_NAME in hd.problems[1]


def test_the_conventions_line_is_no_attribute(tmp_path):
    path = str(tmp_path / "r.bin")
    for style in ("gfortran", "compact"):
        rr.write_header(path, globals_(), FIELDS, style=style, conventions="CF-1.0")
        hd = rr.read_header(path)
        assert hd.problems == [] and hd.conventions is None
        assert rr.CONVENTIONS_NAME not in hd.attrs and "conventions" not in hd.attrs
        assert [ln for ln in hd.ignored if "CF-1.0" in ln] == [rr.CONVENTIONS_NAME + ":" + (" " if style == "gfortran" else "") + "CF-1.0"]
    # a colon in its value gives it a second separator, and a "type" nobody knows: still ignored
    rr.write_header(path, globals_(), FIELDS, conventions="CF:1.0")
    hd = rr.read_header(path)
    assert hd.problems == [] and hd.conventions is None and rr.CONVENTIONS_NAME not in hd.attrs and len(hd.ignored) == 1
    # an undamaged line is taken
    with open(path + ".hdr", "w") as h:
        h.write("&GLOBAL\nconventions:char: CF-1.0\n/\n")
    assert rr.read_header(path).conventions == "CF-1.0"


def test_what_the_reference_would_stop_at(tmp_path):
    path = str(tmp_path / "r.bin")
    with open(path + ".hdr", "w") as h:
        h.write("&GLOBAL\nnsteps_total:int: 12.5\neod:log: maybe\ndtt:r8: fast\nempty:int:\nodd:complex: (1,2)\nok:LOGICAL: .true.\nd:dbl: 1.5D+02\n/\n")
        h.write("&A\nid:int: 1\nextra:quad: 1\n/\n&B\nid:int: x\n/\n&C\nid:int: 3\nfine:integer: 4\n")
    hd = rr.read_header(path, fields=["A", "B", "C", "D"])
    assert len(hd.problems) == 8 and hd.ignored == ["odd:complex: (1,2)"]
    assert hd.attrs == {"ok": ("log", True), "d": ("r8", 150.0)} and hd.fields == {}
    for frag in ("nsteps_total", "eod", "dtt", "empty", "unknown data type 'quad'", "id of B", "no '/' ends the section of C", "find field in binary header file: D"):
        assert any(frag in p for p in hd.problems), frag
    assert rr.parse_value("log", " .FALSE.") is False and rr.parse_value("log", "Tr") is True and rr.parse_value("int", " +7, 8") == 7
    assert rr.parse_value("r8", " 1.5+3 /") == 1500.0 and rr.parse_value("r8", "-.5e-1") == -0.05 and rr.parse_value("r8", "3600") == 3600.0
    for typ, text in (("int", "7.0"), ("int", ""), ("r8", "1.5x"), ("log", "yes"), ("r8", ",")):
        with pytest.raises(rr.HeaderError):
            rr.parse_value(typ, text)


def test_reference_names():
    names = [n for n, _, _ in globals_()]
    assert len(names) == len(set(names)) == 52 + 4 + KM and all(rr.is_reference_name(n) for n in names)
    assert rr.is_reference_name("title") and rr.is_reference_name("rf_Svol_prev_IAGE") and rr.is_reference_name("sal_initial016")
    for n in ("nsteps_this_interval", "TRACER03_CUR", "sal_initial16", "rf_S_prev_", "eod_next"):
        assert not rr.is_reference_name(n), n
