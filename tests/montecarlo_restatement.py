"""Functions of core/montecarlo.dart restated in plain Python, once, for the test side's restatements of the samplers
(tests/stratified_restatement.py, tests/halton_restatement.py): written apart from dartray_amd.core and from the kernels, cited by
file.dart:line of the reference.  A "Float32List" is a numpy float32 array (a store rounds the f64 expression to f32); rng is anything
with the reference RNG's randomFloat() / randomUint()."""
ONE_MINUS_EPSILON = 0.9999999403953552  # montecarlo.dart:23


def LatinHypercube(samples, nSamples, nDim, rng):                  # montecarlo.dart:305-325 (samples: a Float32List)
    delta = 1.0 / nSamples
    for i in range(nSamples):
        for j in range(nDim):
            samples[nDim * i + j] = min((i + rng.randomFloat()) * delta, ONE_MINUS_EPSILON)
    for i in range(nDim):
        for j in range(nSamples):
            other = j + (rng.randomUint() % (nSamples - j))
            samples[nDim * j + i], samples[nDim * other + i] = samples[nDim * other + i], samples[nDim * j + i]
