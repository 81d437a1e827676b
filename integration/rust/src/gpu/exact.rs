//! The sequential-scan plans on the engine: exact k-NN and range scans over the rows as stored (include/hnswrx.h: hx_exact_search*,
//! hx_exact_range*).
use std::os::raw::c_int;

use super::ffi::*;

/// The `LIMIT k` rows of one query: engine row ids nearest first with the operator's float8 values.
pub struct ExactRows {
    pub ids: Vec<u32>,
    pub distances: Vec<f64>,
}

/// `WHERE cond_i ORDER BY v <op> q_i LIMIT k` for the engine's query slots `0..filter_of.len()` over all stored rows, in one call.
/// `filters[f]`: a row bitmap of `ceil(hx_num_rows / 64)` words; `filter_of[i]`: the filter of query `i`, `None` for no `WHERE`.
/// The executor batches the pending scans of many backends (one tenant predicate each) and splits batches with more than
/// `HX_EXACT_MAX_FILTERS` distinct filters.
pub fn exact_search_filtered_gpu(e: *mut hx_engine, op: c_int, k: u32, filters: &[&[u64]], filter_of: &[Option<usize>]) -> Vec<ExactRows> {
    assert!(filters.len() <= HX_EXACT_MAX_FILTERS as usize, "split the call: more than HX_EXACT_MAX_FILTERS filters");
    let nq = filter_of.len();
    let n_rows = unsafe { hx_num_rows(e) };
    let words = ((n_rows + 63) / 64) as usize;
    assert!(filters.iter().all(|f| f.len() >= words), "a filter needs ceil(n_rows / 64) words");
    let ptrs: Vec<*const u64> = filters.iter().map(|f| f.as_ptr()).collect();
    let of: Vec<i32> = filter_of
        .iter()
        .map(|f| match f {
            None => -1,
            Some(f) => {
                assert!(*f < filters.len(), "filter_of names a filter that is not there");
                *f as i32
            }
        })
        .collect();
    let mut ids = vec![0u32; nq * k as usize];
    let mut dist = vec![0f64; nq * k as usize];
    let mut counts = vec![0u32; nq];
    unsafe {
        ck(
            e,
            hx_exact_search_filtered(e, op, 0, nq as u32, 0, n_rows, ptrs.len() as u32, ptrs.as_ptr(), of.as_ptr(), k, ids.as_mut_ptr(),
                                     dist.as_mut_ptr(), counts.as_mut_ptr()),
        );
    }
    (0..nq)
        .map(|q| {
            let (a, b) = (q * k as usize, q * k as usize + counts[q] as usize);
            ExactRows { ids: ids[a..b].to_vec(), distances: dist[a..b].to_vec() }
        })
        .collect()
}

/// `WHERE cond_i AND v <op> q_i <cmp> r_i` (`order`: `HX_RANGE_BY_ROW`, or `HX_RANGE_BY_DISTANCE` for `ORDER BY v <op> q_i` without LIMIT) for the
/// engine's query slots `0..filter_of.len()` over all stored rows, in one call; `filters` and `filter_of` as in `exact_search_filtered_gpu`.
/// Returns per query its rows and their values.  A first call counts (`SELECT count(*)` stops there), the second is sized to the total.
pub fn exact_range_filtered_gpu(e: *mut hx_engine, op: c_int, cmp: c_int, radius: &[f64], filters: &[&[u64]], filter_of: &[Option<usize>],
                                order: c_int) -> Vec<ExactRows> {
    assert!(filters.len() <= HX_EXACT_MAX_FILTERS as usize, "split the call: more than HX_EXACT_MAX_FILTERS filters");
    let nq = filter_of.len();
    assert!(radius.len() == nq, "one radius per query");
    let n_rows = unsafe { hx_num_rows(e) };
    let words = ((n_rows + 63) / 64) as usize;
    assert!(filters.iter().all(|f| f.len() >= words), "a filter needs ceil(n_rows / 64) words");
    let ptrs: Vec<*const u64> = filters.iter().map(|f| f.as_ptr()).collect();
    let of: Vec<i32> = filter_of
        .iter()
        .map(|f| match f {
            None => -1,
            Some(f) => {
                assert!(*f < filters.len(), "filter_of names a filter that is not there");
                *f as i32
            }
        })
        .collect();
    let mut offsets = vec![0u64; nq + 1];
    let mut total = 0u64;
    unsafe {
        ck(
            e,
            hx_exact_range_filtered(e, op, cmp, radius.as_ptr(), 0, nq as u32, 0, n_rows, ptrs.len() as u32, ptrs.as_ptr(), of.as_ptr(), order, 0,
                                    offsets.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut(), &mut total),
        );
    }
    let mut ids = vec![0u32; total as usize];
    let mut dist = vec![0f64; total as usize];
    unsafe {
        ck(
            e,
            hx_exact_range_filtered(e, op, cmp, radius.as_ptr(), 0, nq as u32, 0, n_rows, ptrs.len() as u32, ptrs.as_ptr(), of.as_ptr(), order, total,
                                    offsets.as_mut_ptr(), ids.as_mut_ptr(), dist.as_mut_ptr(), &mut total),
        );
    }
    (0..nq)
        .map(|q| {
            let (a, b) = (offsets[q] as usize, offsets[q + 1] as usize);
            ExactRows { ids: ids[a..b].to_vec(), distances: dist[a..b].to_vec() }
        })
        .collect()
}

/// The tenant column of a table as a filter set: made when the host first sees the table (`labels[i]`: the tenant number of row `i`,
/// `HX_NO_LABEL` for a NULL tenant), extended by `filterset_append_gpu` on insert, dropped and rebuilt after a vacuum that renumbers rows.
pub fn filterset_from_labels_gpu(e: *mut hx_engine, labels: &[u32], n_filters: u32) -> *mut hx_filterset {
    let mut s: *mut hx_filterset = std::ptr::null_mut();
    unsafe { ck(e, hx_filterset_create_labels(e, 0, labels.len() as u64, n_filters, labels.as_ptr(), &mut s)) };
    s
}

/// The labels of the rows appended to the engine since the set was made or last extended.
pub fn filterset_append_gpu(e: *mut hx_engine, s: *mut hx_filterset, labels: &[u32]) {
    unsafe { ck(e, hx_filterset_append_labels(s, labels.len() as u64, labels.as_ptr())) };
}

fn filter_of_set(filter_of: &[Option<u32>]) -> Vec<i32> {
    filter_of.iter().map(|f| f.map_or(-1, |f| f as i32)).collect()
}

/// `exact_search_filtered_gpu` over the rows the set covers, the set's resident lists standing for the bitmaps: `filter_of[i]` is query `i`'s
/// tenant number, `None` for no `WHERE`.  The executor splits batches that name more than `HX_EXACT_MAX_FILTERS` distinct tenants.
pub fn exact_search_set_gpu(e: *mut hx_engine, op: c_int, k: u32, s: *const hx_filterset, filter_of: &[Option<u32>]) -> Vec<ExactRows> {
    let nq = filter_of.len();
    let of = filter_of_set(filter_of);
    let mut ids = vec![0u32; nq * k as usize];
    let mut dist = vec![0f64; nq * k as usize];
    let mut counts = vec![0u32; nq];
    unsafe {
        ck(e, hx_exact_search_set(e, op, 0, nq as u32, s, of.as_ptr(), k, ids.as_mut_ptr(), dist.as_mut_ptr(), counts.as_mut_ptr()));
    }
    (0..nq)
        .map(|q| {
            let (a, b) = (q * k as usize, q * k as usize + counts[q] as usize);
            ExactRows { ids: ids[a..b].to_vec(), distances: dist[a..b].to_vec() }
        })
        .collect()
}

/// `exact_range_filtered_gpu` over the rows the set covers, the set's resident lists standing for the bitmaps.
pub fn exact_range_set_gpu(e: *mut hx_engine, op: c_int, cmp: c_int, radius: &[f64], s: *const hx_filterset, filter_of: &[Option<u32>],
                           order: c_int) -> Vec<ExactRows> {
    let nq = filter_of.len();
    assert!(radius.len() == nq, "one radius per query");
    let of = filter_of_set(filter_of);
    let mut offsets = vec![0u64; nq + 1];
    let mut total = 0u64;
    unsafe {
        ck(
            e,
            hx_exact_range_set(e, op, cmp, radius.as_ptr(), 0, nq as u32, s, of.as_ptr(), order, 0, offsets.as_mut_ptr(), std::ptr::null_mut(),
                               std::ptr::null_mut(), &mut total),
        );
    }
    let mut ids = vec![0u32; total as usize];
    let mut dist = vec![0f64; total as usize];
    unsafe {
        ck(
            e,
            hx_exact_range_set(e, op, cmp, radius.as_ptr(), 0, nq as u32, s, of.as_ptr(), order, total, offsets.as_mut_ptr(), ids.as_mut_ptr(),
                               dist.as_mut_ptr(), &mut total),
        );
    }
    (0..nq)
        .map(|q| {
            let (a, b) = (offsets[q] as usize, offsets[q + 1] as usize);
            ExactRows { ids: ids[a..b].to_vec(), distances: dist[a..b].to_vec() }
        })
        .collect()
}
