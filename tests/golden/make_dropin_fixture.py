#!/usr/bin/env python3
"""Record what the reference's own liboqs wrapper and KEM plugins see over libqrkem.so into
tests/golden/dropin.json.

Runs ONLY in the build container (needs /root/reference and a built libqrkem.so; no GPU):
loads the reference's quantum_resistant_p2p/vendor/oqs.py unmodified, pointed at a temporary
$OQS_INSTALL_PATH/lib/liboqs.so symlink to libqrkem.so (its documented fallback), then its
crypto/key_exchange.py over that wrapper, and stores what they report: the version string,
the supported / enabled mechanism lists, every enabled KEM's `details`, the exceptions for
names the library refuses, the plugins' variant per level, and the errors the wrapper raises
when no HIP device is present.  tests/test_abi.py checks the same facts on the library through
qrkem's own binding.  Only outputs are stored; no reference source is copied.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import tempfile
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
REF = Path("/root/reference/quantum_resistant_p2p")
OUT = Path(__file__).resolve().parent / "dropin.json"
sys.path.insert(0, str(ROOT / "quantum-resistant-p2p_amd"))

REFUSED = ["BIKE-L1", "Kyber768", "NoSuchKEM"]


def outcome(fn):
    try:
        fn()
        return "ok"
    except Exception as exc:  # noqa: BLE001
        return f"{type(exc).__name__}: {exc}"


def main():
    import qrkem
    assert qrkem.device_count() == 0, "record the no-device errors on a host without a GPU"
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "lib"))
        os.symlink(qrkem.LIB_PATH, os.path.join(d, "lib", "liboqs.so"))
        os.environ["OQS_INSTALL_PATH"] = d
        spec = importlib.util.spec_from_file_location("ref_vendor_oqs", REF / "vendor" / "oqs.py")
        oqs = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(oqs)
    out = {"version": oqs.oqs_version(), "supported": list(oqs.get_supported_kem_mechanisms()),
           "enabled": list(oqs.get_enabled_kem_mechanisms()),
           "enabled_sigs": list(oqs.get_enabled_sig_mechanisms()), "details": {}, "refused": {}}
    for name in out["enabled"]:
        k = oqs.KeyEncapsulation(name)
        out["details"][name] = k.details
        k.free()
    for name in REFUSED:
        out["refused"][name] = outcome(lambda n=name: oqs.KeyEncapsulation(n)).split(":")[0]
    k = oqs.KeyEncapsulation("ML-KEM-768")
    out["no_device"] = {"generate_keypair": outcome(k.generate_keypair),
                        "encap_secret": outcome(lambda: k.encap_secret(bytes(k.details["length_public_key"])))}
    k2 = oqs.KeyEncapsulation("ML-KEM-768", bytes(k.details["length_secret_key"]))
    out["no_device"]["decap_secret"] = outcome(lambda: k2.decap_secret(bytes(k.details["length_ciphertext"])))
    out["no_device"]["last_error"] = qrkem.last_error()
    sys.modules["oqs"] = oqs
    pkg = types.ModuleType("refcrypto2")
    pkg.__path__ = [str(REF / "crypto")]
    sys.modules["refcrypto2"] = pkg
    for name in ("algorithm_base", "key_exchange"):
        spec = importlib.util.spec_from_file_location(f"refcrypto2.{name}", REF / "crypto" / f"{name}.py")
        m = importlib.util.module_from_spec(spec)
        sys.modules[f"refcrypto2.{name}"] = m
        spec.loader.exec_module(m)
    ke = sys.modules["refcrypto2.key_exchange"]
    out["plugins"] = []
    for cls, kw in ([("MLKEMKeyExchange", {"security_level": lv}) for lv in (1, 3, 5)]
                    + [("HQCKeyExchange", {"security_level": lv}) for lv in (1, 3, 5)]
                    + [("FrodoKEMKeyExchange", {"security_level": lv, "use_aes": aes}) for lv in (1, 3, 5)
                       for aes in (True, False)]):
        obj = getattr(ke, cls)(**kw)
        out["plugins"].append({"cls": cls, "kwargs": kw, "name": obj.name, "variant": obj.variant,
                               "generate_keypair": outcome(obj.generate_keypair)})
    OUT.write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
