"""CPU tests of the binding itself: wmix_amd/_lib.py reads every ctypes signature from include/*.h (one parser; no hand
table), binds all of them on the library and fails loudly on anything it cannot type.  No compute calls; no GPU needed."""
import ctypes as C
import subprocess

import pytest

from wmix_amd import _lib
from wmix_amd._lib import WMix_Point, WMix_Struct_Head, WmxError

vp, i, u, lg, sz = C.c_void_p, C.c_int, C.c_uint, C.c_long, C.c_size_t
u8, u16, u32 = C.c_uint8, C.c_uint16, C.c_uint32

# one signature per type class, written out from the headers by hand
BY_HAND = {
    "wmx_ns_process": (i, [vp, vp, vp, i, lg, lg, vp]),  # long strides
    "wmx_chain_create": (i, [vp, i, i, i, i, i, u, i]),  # unsigned
    "wmx_mix_load": (i, [vp, vp, u32, i, i, i, i, lg, lg, i, vp, vp, vp]),  # uint32_t scalars and out-pointers
    "wmx_last_error": (C.c_char_p, []),  # const char * return
    "wmx_pipe_in": (vp, [vp, i]),  # pointer return
    "wmx_pipe_failed_steps": (lg, [vp]),  # long return
    "aec_release": (None, [vp]),  # void return
    "wmix_len_of_out": (u32, [u8, u16, u32, u8, u16]),  # uint8_t / uint16_t scalars
    "linear2alaw": (C.c_ubyte, [i]),  # unsigned char return
    "wmx_aec_timing": (i, [vp, vp, vp, vp]),  # int * / double * results
    "wmx_g711_encode": (i, [i, vp, vp, sz, vp]),  # size_t
    "wmix_load_data": (WMix_Point, [vp, WMix_Point, u32, u16, u8, u8, WMix_Point, u8, vp]),  # by-value union
    "g711a_decode": (i, [vp, vp, i]),  # name[] parameters
    "FFTR": (None, [vp] * 6 + [u]),  # unsigned int
    "wmx_version": (i, []),  # (void)
}


def test_every_declared_symbol_has_a_signature():
    table = _lib.signatures()
    names = _lib.declared_symbols()
    assert names == sorted(table) and len(names) >= 240
    for n in names:
        restype, argtypes = table[n]
        assert isinstance(argtypes, list), n
        assert restype is None or isinstance(restype, type), n
        assert all(isinstance(a, type) for a in argtypes), n


@pytest.mark.parametrize("name", sorted(BY_HAND))
def test_parsed_signature_equals_the_one_written_by_hand(name):
    assert _lib.signatures()[name] == BY_HAND[name]


def test_library_is_bound_with_the_parsed_signatures(wmx):
    assert _lib.unbound == []
    for n, (restype, argtypes) in _lib.signatures().items():
        f = getattr(wmx, n)
        assert f.restype is restype and f.argtypes == argtypes, n


def test_symbols_the_library_lacks_are_listed_not_bound():
    """a variant library built from an older tree: the names it does not export go to `unbound`, the rest are bound"""
    class Fn:
        pass

    class Older:
        wmx_version, wmx_last_error = Fn(), Fn()

    saved = list(_lib.unbound)
    try:
        _lib._bind(Older)
        assert sorted(_lib.unbound) == [n for n in _lib.declared_symbols() if n not in ("wmx_version", "wmx_last_error")]
        assert Older.wmx_last_error.restype is C.c_char_p and Older.wmx_last_error.argtypes == []
    finally:
        _lib.unbound[:] = saved


@pytest.mark.parametrize("text,token", [
    ("int wmx_ok(int a);\nint wmx_bad(int a, wchar_t b);", "wchar_t"),  # an unknown scalar type
    ("typedef struct { int a; } Pair;\nPair wmx_bad(int a);", "Pair"),  # a by-value aggregate not in the registry
    ("int wmx_bad(Pair p, int a);", "Pair"),
    ("int wmx_bad(void *h, void (*done)(void *, int), void *arg);", "(*done)"),  # a function-pointer parameter
    ("int wmx_bad(unsigned long);", "unsigned long"),
    ("long long wmx_bad(void);", "long long"),
    ("int wmx_bad();", ""),
])
def test_parser_refuses_what_it_cannot_type(text, token):
    with pytest.raises(WmxError) as e:
        _lib.parse_prototypes(text)
    assert "wmx_bad" in str(e.value) and token in str(e.value) and "wmx_ok" not in str(e.value)


def test_parser_refuses_what_is_not_a_prototype():
    with pytest.raises(WmxError):
        _lib.parse_prototypes("extern int wmx_counter;")


def test_parser_reads_the_forms_the_headers_use():
    text = """/* a comment with a call(in, it); */
    #define WMX_F(x) ((x) + 1)
    #ifdef __cplusplus
    extern "C" {
    #endif
    typedef struct wmx_t wmx_t;
    typedef union { int8_t *S8; } WMix_Point; // another comment(s);
    const char *name_of(void);
    const uint8_t *rows(wmx_t *h, int slot);
    unsigned kinds(const wmx_t *h, unsigned int, unsigned n, const float x[], bool *debug,
                   long stride);
    WMix_Point load(WMix_Point src, uint8_t reduce);
    #ifdef __cplusplus
    }
    #endif
    """
    assert _lib.parse_prototypes(text) == {"name_of": (C.c_char_p, []), "rows": (vp, [vp, i]), "kinds": (u, [vp, u, u, vp, vp, lg]),
                                           "load": (WMix_Point, [WMix_Point, u8])}


def test_missing_header_directory_is_an_error(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_signatures", None)
    monkeypatch.setattr(_lib, "INCLUDE_DIR", str(tmp_path / "nowhere"))
    with pytest.raises(WmxError) as e:
        _lib.signatures()
    assert "nowhere" in str(e.value)


def test_aggregates_have_the_layout_the_compiler_gives_them(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wmix_compat.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(WMix_Point), sizeof(WMix_Struct_Head), '
                   'offsetof(WMix_Struct_Head, tick), offsetof(WMix_Struct_Head, reduceMode)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + _lib.INCLUDE_DIR, str(src), "-o", str(exe)])
    want = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert [C.sizeof(WMix_Point), C.sizeof(WMix_Struct_Head), WMix_Struct_Head.tick.offset, WMix_Struct_Head.reduceMode.offset] == want
