"""Access to the stored test vectors under ``tests/golden/``.

A vector larger than the repository's per-file size limit is stored as ``<name>.part0``,
``<name>.part1``, ... (a plain byte split); :func:`read_parts` joins them again.
"""
import atexit
import glob
import os
import shutil
import tempfile

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MNIST_RAW = os.path.join(GOLDEN, "mnist", "MNIST", "raw")
_MNIST_ENV = "EWDML_GOLDEN_MNIST"


def read_parts(path: str) -> bytes:
    """The bytes of ``path``, stored whole or as ``path.part<i>``."""
    if os.path.exists(path):
        with open(path, "rb") as f:
            return f.read()
    parts = sorted(glob.glob(path + ".part*"), key=lambda p: int(p.rsplit(".part", 1)[1]))
    if not parts:
        raise FileNotFoundError(path)
    data = b""
    for p in parts:
        with open(p, "rb") as f:
            data += f.read()
    return data


def mnist_root() -> str:
    """A ``--data-dir`` holding the 10,000 MNIST test images and labels in the layout the dataset
    reader expects (``<root>/MNIST/raw/t10k-*.gz``).  The image file is stored in parts, so the
    directory is assembled once in a temporary location; child processes find it through the
    environment, and the process that made it removes it at exit."""
    root = os.environ.get(_MNIST_ENV)
    if root and os.path.isdir(os.path.join(root, "MNIST", "raw")):
        return root
    root = tempfile.mkdtemp(prefix="ewdml_mnist_")
    raw = os.path.join(root, "MNIST", "raw")
    os.makedirs(raw)
    with open(os.path.join(raw, "t10k-images-idx3-ubyte.gz"), "wb") as f:
        f.write(read_parts(os.path.join(MNIST_RAW, "t10k-images-idx3-ubyte.gz")))
    shutil.copy(os.path.join(MNIST_RAW, "t10k-labels-idx1-ubyte.gz"), raw)
    os.environ[_MNIST_ENV] = root
    atexit.register(shutil.rmtree, root, ignore_errors=True)
    return root
