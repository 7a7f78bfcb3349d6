"""Record sklearn's k-means results for the cases of tests/oracle_kmeans.py into
tests/golden/kmeans.npz (needs scikit-learn; the recorded file was made with 1.7.2).

The inputs are regenerated from their seeds (oracle_kmeans.lloyd_case / pp_case); only what sklearn
returned is stored: labels_, cluster_centers_, inertia_, n_iter_ of KMeans(init=centres, n_init=1)
and the indices of sklearn.cluster.kmeans_plusplus.

    python tools/make_kmeans_golden.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import sklearn
    from sklearn.cluster import KMeans, kmeans_plusplus
    import oracle_kmeans as ok
    out = {'sklearn_version': np.array(sklearn.__version__)}
    for case in ok.LLOYD_CASES:
        name, N, E, K, seed, tol, max_iter, far = case
        x, init = ok.lloyd_case(case)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')  # max_iter cases end without convergence on purpose
            km = KMeans(n_clusters=K, init=init, n_init=1, max_iter=max_iter, tol=tol).fit(x)
        out[f'lloyd/{name}/labels'] = km.labels_.astype(np.int32)
        out[f'lloyd/{name}/centers'] = km.cluster_centers_.astype(np.float64)
        out[f'lloyd/{name}/inertia'] = np.float64(km.inertia_)
        out[f'lloyd/{name}/n_iter'] = np.int32(km.n_iter_)
    for i, case in enumerate(ok.PP_CASES):
        N, E, K, seed, pp_seed = case
        _, indices = kmeans_plusplus(ok.pp_case(case), K, random_state=pp_seed)
        out[f'pp/{i}/indices'] = indices.astype(np.int32)
    path = os.path.join(ROOT, 'tests', 'golden', 'kmeans.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
