"""The reference package (h3jia/bayesfast: Python with four Cython extensions), built from a read-only checkout of it into
``oracle/_ref/`` for the CPU tests that drive the reference's own code (tests/test_integrate_reference.py) and for the fixture
and timing scripts (tests/golden/make_golden.py, tools/time_reference.py).

``oracle/_ref/`` is a build product and stays out of git: nothing of the reference's source enters the repository.
``build()`` (``__graft_entry__.build``) fills it when the checkout exists (``BF_REFERENCE``, default /root/reference) and
leaves it alone otherwise; the tests that need it are skipped where it was never built.  The reference's own tests are not
copied, so that no test collector finds them in the tree."""
import os
import shutil
import subprocess
import sys
import types

import numpy as np

REF_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_ref')

BUILD_EXT = r'''
import numpy as np
from setuptools import setup, Extension
from Cython.Build import cythonize
names = ['bayesfast/modules/_poly', 'bayesfast/transforms/_constraint', 'bayesfast/utils/_sobol',
         'bayesfast/utils/_cubic']
exts = [Extension(n.replace('/', '.'), [n + '.pyx'], include_dirs=[np.get_include()],
                  extra_compile_args=['-fopenmp', '-O3'], extra_link_args=['-fopenmp']) for n in names]
setup(ext_modules=cythonize(exts, language_level='3'))
'''


def source():
    """The reference checkout to build from."""
    return os.environ.get('BF_REFERENCE', '/root/reference')


def is_built(work=REF_DIR):
    mod = os.path.join(work, 'bayesfast', 'modules')
    return os.path.isdir(mod) and any(f.endswith('.so') for f in os.listdir(mod))


def build(ref=None, work=REF_DIR):
    """Copy the reference package to ``work`` and build its Cython extensions in place (a no-op when they are built).  Returns
    False when there is neither a build nor a checkout to build from."""
    if is_built(work):
        return True
    ref = ref or source()
    if not os.path.isdir(os.path.join(ref, 'bayesfast')):
        return False
    pkg = os.path.join(work, 'bayesfast')
    os.makedirs(work, exist_ok=True)
    if os.path.exists(pkg):
        shutil.rmtree(pkg)
    shutil.copytree(os.path.join(ref, 'bayesfast'), pkg, ignore=shutil.ignore_patterns('tests', '__pycache__'))
    with open(os.path.join(work, 'build_ext.py'), 'w') as f:
        f.write(BUILD_EXT)
    r = subprocess.run([sys.executable, 'build_ext.py', 'build_ext', '--inplace'], cwd=work, capture_output=True, text=True)
    if r.returncode != 0:   # (the compilers' warnings are shown only when the build fails)
        raise RuntimeError('building the reference failed:\n' + r.stderr[-3000:])
    return True


def load(work=REF_DIR):
    """Import the reference built in ``work`` behind two environment shims, and return its top-level package."""
    # shim 1: NumPy aliases removed in 1.24 that the reference still uses
    for n, t in (('int', int), ('float', float)):
        if not hasattr(np, n):
            setattr(np, n, t)
    # shim 2: numdifftools is not installed; only Laplace (OptimizeStep) and the reference's tests use it
    nd = types.ModuleType('numdifftools')

    def _central(f, x, h=1e-6):
        x = np.atleast_1d(np.asarray(x, dtype=float))
        f0 = np.atleast_1d(f(x))
        J = np.empty((f0.size, x.size))
        for i in range(x.size):
            e = np.zeros_like(x)
            e[i] = h
            J[:, i] = (np.atleast_1d(f(x + e)) - np.atleast_1d(f(x - e))) / (2 * h)
        return J

    class Gradient:
        def __init__(self, f, *a, **k):
            self.f = f

        def __call__(self, x):
            return _central(self.f, x)[0]

    class Jacobian(Gradient):
        def __call__(self, x):
            return _central(self.f, x)

    class Hessian(Gradient):
        def __call__(self, x):
            return _central(lambda y: _central(self.f, y)[0], x, 1e-4)

    class Hessdiag(Gradient):
        def __call__(self, x):
            return np.diag(Hessian(self.f)(x))

    nd.Gradient, nd.Jacobian, nd.Hessian, nd.Hessdiag = Gradient, Jacobian, Hessian, Hessdiag
    sys.modules['numdifftools'] = nd
    sys.path.insert(0, work)
    import bayesfast  # noqa: F401
    return bayesfast
