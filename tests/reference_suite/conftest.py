"""Tests that use the drop-in under the reference's package name: `dex_retargeting` and every `dex_retargeting.<module>` are
aliased to `dex_retargeting_amd` in sys.modules BEFORE collection.  The directory layout code written against the reference
expects (<here>/assets/robots/hands, <here>/dex_retargeting/configs, <here>/src/dex_retargeting/configs) is committed as
relative symlinks to the package's own assets/ and configs/."""
import importlib
import os
import pkgutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
sys.path.insert(0, HERE)


def alias_package():
    import dex_retargeting_amd as pkg

    sys.modules["dex_retargeting"] = pkg
    for m in pkgutil.iter_modules(pkg.__path__):
        if m.name.startswith("_") or m.ispkg or not os.path.exists(os.path.join(pkg.__path__[0], m.name + ".py")):
            continue  # python modules only (libdexr.so sits in the package directory too)
        sys.modules[f"dex_retargeting.{m.name}"] = importlib.import_module(f"dex_retargeting_amd.{m.name}")


alias_package()
