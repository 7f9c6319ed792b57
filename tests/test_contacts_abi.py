"""Contact readout, host side (no GPU): mjl_model_ncon_max, the binding of mjl_forward_contacts as the
header declares it, Model.ncon_max, and the argument errors that are reported before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mjx_amd
from mjx_amd import _lib, abi
from mjx_amd._header import HEADER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model_handle(name):
    m = mjx_amd.load_model(name)
    h = C.c_void_p()
    assert _lib.lib().mjl_model_create(C.byref(abi.model_desc(m)), C.byref(h)) == 0
    return m, h


@pytest.mark.parametrize("name", mjx_amd.BUILTIN_MODELS)
def test_ncon_max_counts_one_contact_per_pair_two_per_plane_capsule(name):
    L = _lib.lib()
    m, h = _model_handle(name)
    kind = np.asarray(m.pair_kind)
    assert L.mjl_model_ncon_max(h) == m.npair + int((kind == HEADER.enums["MJL_COL_PLANE_CAPSULE"]).sum())
    assert L.mjl_model_ncon_max(h) >= 1
    L.mjl_model_destroy(h)


def test_ncon_max_of_a_null_model():
    assert _lib.lib().mjl_model_ncon_max(None) == -1


def test_binding_has_the_headers_argument_lists():
    """Both functions are bound with the argument lists written in include/mjx355.h (read here with this
    test's own regex): a model handle; batch, mask, max_con, five int32 and five float buffers, stream."""
    hdr = open(os.path.join(ROOT, "include", "mjx355.h")).read()
    protos = dict((n, a) for n, a in re.findall(r"^int\s+(mjl_model_ncon_max|mjl_forward_contacts)\(([^)]*)\)", hdr, re.M))
    assert set(protos) == {"mjl_model_ncon_max", "mjl_forward_contacts"}
    names = [a.split()[-1].lstrip("*") for a in protos["mjl_forward_contacts"].split(",")]
    assert names == ["batch", "mask", "max_con", "ncon", "geom", "dim", "efc_adr", "dist", "pos", "frame", "force",
                     "body_force", "stream"]
    L = _lib.lib()
    vp, i32 = C.c_void_p, C.c_int
    assert "mjl_model_ncon_max" in _lib.EXPORTS and "mjl_forward_contacts" in _lib.EXPORTS
    assert L.mjl_model_ncon_max.argtypes == [vp] and L.mjl_model_ncon_max.restype is i32
    assert L.mjl_forward_contacts.argtypes == [vp, vp, i32] + [vp] * 10 and L.mjl_forward_contacts.restype is i32
    by_name = {n: a for _, n, a in HEADER.protos}
    assert by_name["mjl_forward_contacts"] == (["mjlBatch*", "float*", "int"] + ["int32_t*"] * 4 + ["float*"] * 5
                                               + ["void*"])


def test_no_field_was_added():
    assert len(abi.FIELD) == 16 and HEADER.enums["MJL_NFIELD"] == 16


@pytest.mark.parametrize("name", mjx_amd.BUILTIN_MODELS)
def test_model_property(name):
    from mjx_amd import mjx
    m = mjx_amd.load_model(name)
    sys_ = mjx.put_model(m)
    assert sys_.ncon_max == _lib.lib().mjl_model_ncon_max(sys_.handle) > 0
    assert sys_.ncon_max <= sys_.nefc_max  # every contact has at least one row


def test_package_exports_the_readout():
    from mjx_amd import mjx
    assert mjx_amd.forward_contacts is mjx.forward_contacts and mjx_amd.Contacts is mjx.Contacts
    assert hasattr(mjx.Contacts, "force_world")


def test_null_batch_is_an_argument_error_without_gpu():
    L = _lib.lib()
    err = HEADER.enums["MJL_ERR_ARG"]
    assert L.mjl_forward_contacts(None, None, 8, *([None] * 10)) == err
    assert b"null batch" in L.mjl_last_error()
