// sect.cc -- `kat sect` (src/sect.cc): k-mer coverage along every record of a sequence file.
//
// The reference walks each record with substr + validKmer + mer_dna + JellyfishHelper::getCount (src/sect.cc:516-535), one
// record per std::thread.  Here a batch of records is joined into one base buffer and profiled by a single
// katgpu_table_profile_host call; what stays on the host is what the reference also does after the lookups: the
// per-record statistics and the text.  When no per-position output is asked for (-n) the device keeps the counts to itself: the
// per-record statistics (katgpu_table_record_stats_host) and the regions of -E / -F (katgpu_table_record_regions_host) come back.
// With KATGPU_SECT_DEVICE_TEXT=1 that holds without -n as well: the lines of -counts.cvg are rendered on the device
// (katgpu_table_record_cvg_text_host) and no count comes back in any one-GPU mode.  In both of these modes the lines of -g's -counts.gc
// come from the device as well (katgpu_record_gc_text_host), so nothing walks a record's bases on the host.  --gpus N with -n does
// the same against a hash that lies on the ranks: one collective per batch (katgpu_table_record_stats_gathered_host) gathers the counts
// on rank 0's device and reduces them there, statistics and regions alike; without -n it gathers the per-position counts on rank 0's host
// (katgpu_table_profile_gathered_host).  Records are read with the semantics of the vendored SeqAn 2.0.0 reader
// (deps/seqan-library-2.0.0/include/seqan/seq_io/fasta_fastq.h:306-380, CharString target).
#include "kat_host.hpp"
#include "record_stats_host.hpp"

#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <thread>

using std::cout;
using std::endl;
using std::string;
using std::vector;

namespace kat {

namespace {
struct PhaseTimer {     // boost::timer::auto_cpu_timer(1, "  Time taken: %ws\n\n")
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    const char* fmt;
    explicit PhaseTimer(const char* f = "  Time taken: %.1fs\n\n") : fmt(f) {}
    ~PhaseTimer() {
        char buf[128];
        snprintf(buf, sizeof buf, fmt, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        cout << buf;
        cout.flush();
    }
};

bool endsWithNoCase(const string& s, const char* suffix) {
    const size_t n = strlen(suffix);
    if (s.size() < n) return false;
    for (size_t i = 0; i < n; i++) if (tolower((unsigned char)s[s.size() - n + i]) != suffix[i]) return false;
    return true;
}

inline void appendU64(string& s, uint64_t v) {
    char tmp[24]; int n = 0;
    do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) s.push_back(tmp[--n]);
}
}  // namespace

// ---- SeqRecordReader: FASTA / FASTQ records the way seqan::SeqFileIn + readRecords deliver them ----
struct SeqRecordReader::Impl {
    gzFile f = nullptr;
    vector<unsigned char> buf = vector<unsigned char>(1 << 20);
    size_t pos = 0, len = 0;
    bool fill() {
        if (pos < len) return true;
        int r = gzread(f, buf.data(), (unsigned)buf.size());
        if (r <= 0) { len = pos = 0; return false; }
        len = (size_t)r; pos = 0;
        return true;
    }
};

SeqRecordReader::SeqRecordReader(const string& path) : impl(new Impl) {
    impl->f = gzopen(path.c_str(), "rb");
    if (!impl->f) throw std::runtime_error("Could not open sequence file: " + path);
    string base = path;
    if (endsWithNoCase(base, ".gz")) base.resize(base.size() - 3);
    // SeqAn decides on the file name alone (fasta_fastq.h:104-143), case-insensitively; anything else is UnknownExtensionError
    if (endsWithNoCase(base, ".fa") || endsWithNoCase(base, ".fasta")) format = FASTA;
    else if (endsWithNoCase(base, ".fq") || endsWithNoCase(base, ".fastq")) format = FASTQ;
    else if (endsWithNoCase(base, ".txt")) format = RAW;
    else throw std::runtime_error("Unknown file extension of " + path + ": iostream error");
}

SeqRecordReader::~SeqRecordReader() { if (impl->f) gzclose(impl->f); }

int SeqRecordReader::peek() { return impl->fill() ? impl->buf[impl->pos] : -1; }
bool SeqRecordReader::atEnd() { return !impl->fill(); }

void SeqRecordReader::line(string* into) {      // readLine / skipLine (seqan/stream/tokenization.h:408-455)
    int c;
    while ((c = peek()) >= 0 && c != '\n' && c != '\r') { if (into) into->push_back((char)c); impl->pos++; }
    if (peek() == '\r') impl->pos++;
    if (peek() == '\n') impl->pos++;
}

void SeqRecordReader::readRecord(string& name, string& seq) { read(name, seq, nullptr); }
void SeqRecordReader::readRecord(string& name, string& seq, string& qual) { read(name, seq, &qual); }

void SeqRecordReader::read(string& name, string& seq, string* qual) {
    name.clear(); seq.clear();
    if (qual) qual->clear();
    if (format == RAW) { line(&seq); return; }                                                  // every line a nameless record
    const bool fastq = format == FASTQ;
    const int begin = fastq ? '@' : '>', stop = fastq ? '+' : '>';
    int c;
    while ((c = peek()) >= 0 && c != begin) impl->pos++;
    if (c < 0) throw std::runtime_error("Unexpected end of input.");                            // seqan::UnexpectedEnd
    impl->pos++;
    line(&name);
    // the sequence runs to the next '>' ('+' in FASTQ) wherever it stands; for a char target only newlines are dropped
    while (impl->fill()) {
        unsigned char* p = impl->buf.data() + impl->pos;
        unsigned char* e = impl->buf.data() + impl->len;
        unsigned char* q = p;
        while (q < e && *q != stop && *q != '\n' && *q != '\r') q++;
        seq.append((const char*)p, (size_t)(q - p));
        impl->pos += (size_t)(q - p);
        if (q == e) continue;
        if (*q == stop) break;
        impl->pos++;
    }
    if (!fastq) return;
    if (peek() != '+') throw std::runtime_error("Unexpected end of input.");
    impl->pos++;
    line(nullptr);                                                                              // optional second id
    size_t left = seq.size();                                                                   // CountDownFunctor over non-newline characters
    while (left && (c = peek()) >= 0) { if (c != '\n' && c != '\r') { left--; if (qual) qual->push_back((char)c); } impl->pos++; }
    while ((c = peek()) >= 0 && c != '@') impl->pos++;
}

// ---- Sect ----
Sect::Sect(const vector<string>& counts_files, const string& seq_file) {                        // src/sect.cc:65-83
    input.setMultipleInputs(counts_files);
    input.index = 1;
    seqFile = seq_file;
    outputPrefix = "kat-sect";
}

void Sect::execute() {                                                                          // src/sect.cc:86-125
    struct stat st;
    if (lstat(seqFile.c_str(), &st) != 0)
        throw SectException("Could not find sequence file at: " + seqFile + "; please check the path and try again.");
    input.validateInput();
    ensureDirectoryExists(parentOfAbsolute(outputPrefix));
    if (input.mode == InputHandler::COUNT) input.count(threads);
    else { input.loadHeader(); input.loadHash(); }
    contamination_mx = Matrix64(gcBins, cvgBins);
    processSeqFile();
    if (input.dumpHash) input.dump(outputPrefix + "-hash.jf" + std::to_string(input.merLen), threads);
    merge();
}

void Sect::merge() {                                                                            // src/sect.cc:246-256
    PhaseTimer timer;
    cout << "Merging matrices ...";     // nothing to merge: one matrix, filled on the host from per-record scalars
    cout << " done.";
    cout.flush();
}

void Sect::save() {                                                                             // src/sect.cc:127-141 (never called by Sect::main)
    PhaseTimer timer;
    cout << "Saving results to disk ...";
    cout.flush();
    std::ofstream os((outputPrefix + "-contamination.mx").c_str());
    printContaminationMatrix(os, seqFile);
    os.close();
    cout << " done.";
    cout.flush();
}

void Sect::printContaminationMatrix(std::ostream& out, const string& seq_file) {               // src/sect.cc:449-463
    out << mme::KEY_TITLE << "Contamination Plot for " << seq_file << " and " << "\"\"" << endl;   // hashFile is never set: boost prints ""
    out << mme::KEY_X_LABEL << "GC%" << endl;
    out << mme::KEY_Y_LABEL << "Average K-mer Coverage" << endl;
    out << mme::KEY_Z_LABEL << "Base Count per bin" << endl;
    out << mme::KEY_NB_COLUMNS << gcBins << endl;
    out << mme::KEY_NB_ROWS << cvgBins << endl;
    out << mme::KEY_MAX_VAL << contamination_mx.getMaxVal() << endl;
    out << mme::KEY_TRANSPOSE << "0" << endl;
    out << mme::MX_META_END << endl;
    contamination_mx.printMatrix(out);
}

// The scalars of a record that follow from its length and four tallies (src/sect.cc:544-600).
void Sect::recordScalars(Record& r, uint64_t nbNonZero, uint64_t nbInvalid, uint64_t gcBases, uint64_t nBases) {
    const uint64_t seqLength = r.seq->size();
    const int64_t nbCounts = (int64_t)seqLength - input.merLen + 1;
    r.length = (uint32_t)seqLength;
    r.nonZero = (uint32_t)nbNonZero;
    r.percentNonZero = nbNonZero == 0 || nbCounts <= 0 ? 0.0 : ((double)nbNonZero / (double)nbCounts) * 100.0;
    r.invalid = (uint32_t)nbInvalid;
    r.percentInvalid = nbInvalid == 0 || nbCounts <= 0 ? 0.0 : ((double)nbInvalid / (double)nbCounts) * 100.0;
    const uint64_t notInvalid = (uint64_t)nbCounts - nbInvalid;
    r.percentNonZeroCorrected = nbNonZero == 0 || notInvalid <= 0 ? 0.0 : ((double)nbNonZero / (double)notInvalid) * 100.0;

    volatile double num = (double)gcBases, den = (double)(seqLength - nBases);                  // run-time division: 0/0 is the x86 default NaN ("-nan")
    r.gc = num / den;

    // src/sect.cc:581-600.  average_cvg is never assigned there, so the coverage bin is 0 with or without
    // --cvg_logscale (uint16_t(-inf) is 0 on x86, like uint16_t(NaN) for the GC bin of an all-N record).
    const double xd = r.gc * gcBins;
    r.mx_x = std::isnan(xd) ? 0 : (uint16_t)xd;
    r.mx_y = 0;
}

// printGCCounts, :352-371; gc[j] = G+C of window j, -1 for an invalid one
void Sect::gcText(Record& r, const vector<int16_t>& gc) {
    const uint16_t k = input.merLen;
    vector<string> pct(k + 1);
    char tmp[32];
    for (uint16_t g = 0; g <= k; g++) { snprintf(tmp, sizeof tmp, "%.1f", ((double)g / (double)k) * 100.0); pct[g] = tmp; }
    string& o = r.gc_txt;
    o += '>'; o += *r.name; o += '\n';
    if (!gc.empty()) {
        for (size_t j = 0; j < gc.size(); j++) { if (j) o += ' '; o += gc[j] < 0 ? string("-0.1") : pct[gc[j]]; }
        o += '\n';
    } else o += "0.0\n";
}

// A record from the device's statistics (katgpu_table_record_stats_host): nothing here is per position.  (The GC line of -g is
// rendered on the device: katgpu_record_gc_text_host in processSeqFile.)
void Sect::processSeqStats(Record& r, const katgpu_record_stats& st) {
    const uint16_t k = input.merLen;
    const string& seq = *r.seq;
    const uint64_t seqLength = seq.size();
    const int64_t nbCounts = (int64_t)seqLength - k + 1;
    r.median = 0; r.mean = 0.0;
    if (nbCounts > 0) {
        r.median = (uint32_t)(double)st.median;
        r.mean = (double)st.sum / (double)nbCounts;
    }
    recordScalars(r, st.non_zero, st.invalid, st.gc_bases, st.n_bases);
}

// Everything the reference's processSeq + print* produce for one record, from the device's per-position counts.
void Sect::processSeq(Record& r, const uint64_t* cnt) {                                         // src/sect.cc:486-603
    const uint16_t k = input.merLen;
    const string& seq = *r.seq;
    const uint64_t seqLength = seq.size();
    const int64_t nbCounts = (int64_t)seqLength - k + 1;
    r.median = 0; r.mean = 0.0;
    const size_t nb = nbCounts > 0 ? (size_t)nbCounts : 0;
    vector<int16_t> gc;
    const katgpu_record_stats st = recordStatsFromCounts(seq.data(), seqLength, k, cnt, &gc);   // (record_stats_host.hpp: shared with Cold under --gpus)
    if (nb) {
        r.median = (uint32_t)(double)st.median;
        r.mean = (double)st.sum / (double)nbCounts;
    }
    recordScalars(r, st.non_zero, st.invalid, st.gc_bases, st.n_bases);

    if (!noCountStats) {                                                                        // printCounts, :328-346
        string& o = r.cvg_txt;
        o.reserve(nb * 2 + r.name->size() + 8);
        o += '>'; o += *r.name; o += '\n';
        if (nb) {
            appendU64(o, cnt[0]);
            for (size_t j = 1; j < nb; j++) { o += ' '; appendU64(o, cnt[j]); }
            o += '\n';
        } else o += "0\n";
    }
    if (outputGCStats) gcText(r, gc);
    if (extractNR) regions(r.nr_txt, r, cnt, nb, 1, minRepeat);
    if (extractR) regions(r.r_txt, r, cnt, nb, minRepeat, maxRepeat);
}

void Sect::regions(string& out, const Record& r, const uint64_t* cnt, size_t nb, uint32_t min_count, uint32_t max_count) {   // printRegions, :373-424
    if (!nb) return;
    const string& seq = *r.seq;
    const uint16_t k = input.merLen;
    const string maxcntstr = max_count > 0 ? string("-") + std::to_string(max_count) : "+";
    uint32_t index = 1, start = 0;
    bool inRegion = false;
    string ss;
    auto header = [&](uint32_t end) {
        out += '>'; out += *r.name;
        out += "___region:" + std::to_string(index++) + "_length:" + std::to_string((uint32_t)(end - start - 1)) + "_pos:" + std::to_string(start + 1) + ":" +
               std::to_string(end) + "_cov:" + std::to_string(min_count) + maxcntstr + "\n";
    };
    for (size_t j = 0; j < nb; j++) {
        const uint64_t c = cnt[j];
        if (c >= min_count && (c <= max_count || max_count == 0)) {
            if (!inRegion) { start = (uint32_t)j; inRegion = true; }
            ss += seq[j];
        } else if (inRegion) {
            const uint32_t end = (uint32_t)(j + k - 1);
            header(end);
            out += ss;
            for (size_t q = j + 1; q < end; q++) out += seq[q];
            out += '\n';
            inRegion = false;
            ss.clear();
        }
    }
    if (inRegion) {
        const uint32_t end = (uint32_t)(nb + k - 1);
        header(end);
        out += ss;
        for (size_t q = nb; q < end; q++) out += seq[q];
        out += '\n';
    }
}

// The bytes of regions() from the record's intervals as the device found them (katgpu_table_record_regions_host): rg[i] is the run
// [start, stop) of window starts, in order.  A run that ends inside the record prints seq[start, stop) and then seq[stop + 1, stop + k - 1)
// -- the base at `stop` is skipped, as in the reference -- and one that reaches the last window prints seq[start, nb + k - 1).
void Sect::regionsText(string& out, const Record& r, const katgpu_region* rg, size_t n_rg, uint32_t min_count, uint32_t max_count) {
    const string& seq = *r.seq;
    const uint16_t k = input.merLen;
    const size_t nb = seq.size() >= k ? seq.size() - k + 1 : 0;
    const string maxcntstr = max_count > 0 ? string("-") + std::to_string(max_count) : "+";
    for (size_t i = 0; i < n_rg; i++) {
        const uint32_t start = (uint32_t)rg[i].start;
        const size_t stop = (size_t)rg[i].stop;
        const uint32_t end = (uint32_t)(stop + k - 1);
        out += '>'; out += *r.name;
        out += "___region:" + std::to_string((uint32_t)(i + 1)) + "_length:" + std::to_string((uint32_t)(end - start - 1)) + "_pos:" + std::to_string(start + 1) + ":" +
               std::to_string(end) + "_cov:" + std::to_string(min_count) + maxcntstr + "\n";
        out.append(seq, rg[i].start, stop - rg[i].start);
        for (size_t q = stop == nb ? nb : stop + 1; q < end; q++) out += seq[q];
        out += '\n';
    }
}

void Sect::processSeqFile() {                                                                   // src/sect.cc:143-244
    PhaseTimer timer;
    cout << "Calculating kmer coverage across sequences ...";
    cout.flush();

    SeqRecordReader reader(seqFile);
    if (verbose) std::cerr << endl;
    // --gpus N: after the exchange a k-mer lives on one rank.  Every rank reads the sequence file and takes part in one collective
    // per batch.  With -n that is katgpu_table_record_stats_gathered_host: the counts are gathered on rank 0's device and reduced
    // there, the statistics and the regions of -E / -F from the same gather.  Without -n it is katgpu_table_profile_gathered_host: the
    // per-position counts arrive on rank 0's host and processSeq makes every output from them.  Rank 0 alone opens the outputs; the other
    // ranks create, truncate and write nothing.
    const bool dist = Engine::dist(), speak = !dist || Engine::speaker();
    std::ofstream count_path_stream, gc_count_path_stream, nr_path_stream, r_path_stream, cvg_gc_stream;
    if (speak) {
        if (!noCountStats) count_path_stream.open((outputPrefix + "-counts.cvg").c_str());
        if (outputGCStats) gc_count_path_stream.open((outputPrefix + "-counts.gc").c_str());
        if (extractNR) nr_path_stream.open((outputPrefix + "-non_repetitive.fa").c_str());
        if (extractR) r_path_stream.open((outputPrefix + "-repetitive.fa").c_str());
        cvg_gc_stream.open((outputPrefix + "-stats.tsv").c_str());
        cvg_gc_stream << "seq_name\tmedian\tmean\tgc%\tseq_length\tkmers_in_seq\tinvalid_kmers\t%_invalid\tnon_zero_kmers\t%_non_zero\t%_non_zero_corrected" << endl;
    }

    // The reference reads 1024 records at a time (BATCH_SIZE, src/sect.hpp:66); the batch only bounds memory there and is
    // invisible in the outputs.  Here a batch is bounded by bases instead, so that one device call has enough to do.
    const size_t BATCH_BASES = (size_t)64 << 20;
    vector<string> names, seqs;
    vector<Record> recs;
    string joined;
    vector<uint64_t> counts, offs, lens;
    vector<katgpu_record_stats> stats;
    // -n: nothing per position is written.  The device reduces the counts per record, and with -E / -F it finds the regions as well
    // (--gpus N: from the gathered counts on rank 0's device).
    // KATGPU_SECT_DEVICE_TEXT=1: the same without -n, the lines of -counts.cvg rendered on the device too, one GPU only (the text kernel
    // looks a window up in the table of its own rank).  It is asked for, not the
    // default: a one-GPU run without -n is pinned to the per-position profile by the suite (tests/test_gpu_record_stats.py).
    const char* dt = getenv("KATGPU_SECT_DEVICE_TEXT");
    const bool cvg_text = !dist && !noCountStats && dt && atoi(dt) != 0, stats_only = noCountStats || cvg_text;
    const bool gc_text = stats_only && outputGCStats;        // -g there: the lines of -counts.gc from the device too, from the bases alone
    vector<katgpu_count_range> ranges;
    if (stats_only && extractNR) ranges.push_back({1, minRepeat});
    if (stats_only && extractR) ranges.push_back({minRepeat, maxRepeat});
    katgpu_region* found = nullptr;
    size_t n_found[2] = {0, 0};
    vector<size_t> first_nr, first_r;                         // a record's regions: [first[i], first[i + 1]) of its range's
    char* cvg = nullptr;                                      // the batch's -counts.cvg lines: record i's is [cvg_off[i], cvg_off[i + 1])
    vector<uint64_t> cvg_off;
    char* gct = nullptr;                                      // the same of -counts.gc
    vector<uint64_t> gct_off;
    uint64_t gc_text_bytes = 0;
    // KATGPU_TIMING: where the phase's wall time goes (reader | joined buffer | device call | per-record host work | text), one line on stderr
    double t_part[5] = {0, 0, 0, 0, 0};
    auto lap = [&, t = std::chrono::steady_clock::now()](int part) mutable {
        const auto now = std::chrono::steady_clock::now();
        t_part[part] += std::chrono::duration<double>(now - t).count();
        t = now;
    };
    while (!reader.atEnd()) {
        if (verbose) std::cerr << "Loading Batch of sequences... ";
        names.clear(); seqs.clear();
        size_t bases = 0;
        while (!reader.atEnd() && bases < BATCH_BASES) {
            names.emplace_back(); seqs.emplace_back();
            reader.readRecord(names.back(), seqs.back());
            bases += seqs.back().size() + 1;
        }
        const size_t n = names.size();
        lap(0);
        if (verbose) std::cerr << "Loaded " << n << " records.  Processing batch... ";

        // analyseBatch(): one device call for every window of every record of the batch
        joined.clear(); joined.reserve(bases);
        offs.assign(n, 0);
        for (size_t i = 0; i < n; i++) { offs[i] = joined.size(); joined += seqs[i]; joined += '\n'; }   // a newline can never be in a record
        lap(1);
        if (stats_only) {
            lens.resize(n); stats.resize(n);
            for (size_t i = 0; i < n; i++) lens[i] = seqs[i].size();
            if (dist) {
                Engine::recordStatsGathered(input.hash, joined.data(), joined.size(), offs.data(), lens.data(), n, input.canonical, ranges.data(),
                                            (uint32_t)ranges.size(), speak ? stats.data() : nullptr, speak ? &found : nullptr, speak ? n_found : nullptr);
                if (!speak) continue;
            } else {
                Engine::check(katgpu_table_record_stats_host(input.hash, joined.data(), joined.size(), offs.data(), lens.data(), n, input.canonical ? 1 : 0, stats.data()));
                if (!ranges.empty())
                    Engine::check(katgpu_table_record_regions_host(input.hash, joined.data(), joined.size(), offs.data(), lens.data(), n, input.canonical ? 1 : 0,
                                                                   ranges.data(), (uint32_t)ranges.size(), &found, n_found));
            }
            if (!ranges.empty()) {
                auto index = [&](vector<size_t>& first, const katgpu_region* rg, size_t m) {      // the regions come sorted by record
                    first.assign(n + 1, 0);
                    for (size_t i = 0; i < m; i++) first[rg[i].record + 1]++;
                    for (size_t i = 0; i < n; i++) first[i + 1] += first[i];
                };
                if (extractNR) index(first_nr, found, n_found[0]);
                if (extractR) index(first_r, found + (extractNR ? n_found[0] : 0), n_found[extractNR ? 1 : 0]);
            }
            if (cvg_text) {
                cvg_off.resize(n + 1);
                Engine::check(katgpu_table_record_cvg_text_host(input.hash, joined.data(), joined.size(), offs.data(), lens.data(), n, input.canonical ? 1 : 0,
                                                                &cvg, cvg_off.data()));
            }
            if (gc_text) {
                gct_off.resize(n + 1);
                Engine::check(katgpu_record_gc_text_host(Engine::ctx(), input.merLen, joined.data(), joined.size(), offs.data(), lens.data(), n, &gct, gct_off.data()));
                gc_text_bytes += gct_off[n];
            }
        } else if (dist) {
            if (speak && counts.size() < joined.size()) counts.resize(joined.size());
            Engine::profileGathered(input.hash, joined.data(), joined.size(), input.canonical, speak ? counts.data() : nullptr);
            if (!speak) continue;
        } else {
            if (counts.size() < joined.size()) counts.resize(joined.size());
            Engine::check(katgpu_table_profile_host(input.hash, joined.data(), joined.size(), input.canonical ? 1 : 0, counts.data()));
        }
        lap(2);

        recs.assign(n, Record());
        for (size_t i = 0; i < n; i++) { recs[i].name = &names[i]; recs[i].seq = &seqs[i]; }
        const unsigned workers = std::max<unsigned>(1, std::min<unsigned>(threads, (unsigned)n));
        auto work = [&](unsigned th) {                                                          // processInterlaced, :477-483
            for (size_t i = th; i < n; i += workers) {
                if (!stats_only) { processSeq(recs[i], counts.data() + offs[i]); continue; }
                processSeqStats(recs[i], stats[i]);
                const katgpu_region* r_found = found + (extractNR ? n_found[0] : 0);
                if (extractNR) regionsText(recs[i].nr_txt, recs[i], found + first_nr[i], first_nr[i + 1] - first_nr[i], 1, minRepeat);
                if (extractR) regionsText(recs[i].r_txt, recs[i], r_found + first_r[i], first_r[i + 1] - first_r[i], minRepeat, maxRepeat);
            }
        };
        if (workers == 1) work(0);
        else {
            vector<std::thread> team;
            for (unsigned th = 0; th < workers; th++) team.emplace_back(work, th);
            for (auto& t : team) t.join();
        }
        katgpu_free_host(found);
        found = nullptr;

        lap(3);
        char line[512];
        for (size_t i = 0; i < n; i++) {
            const Record& r = recs[i];
            if (cvg_text) { count_path_stream << '>' << *r.name << '\n'; count_path_stream.write(cvg + cvg_off[i], (std::streamsize)(cvg_off[i + 1] - cvg_off[i])); }
            else if (!noCountStats) count_path_stream << r.cvg_txt;
            if (gc_text) { gc_count_path_stream << '>' << *r.name << '\n'; gc_count_path_stream.write(gct + gct_off[i], (std::streamsize)(gct_off[i + 1] - gct_off[i])); }
            else if (outputGCStats) gc_count_path_stream << r.gc_txt;
            if (extractNR) nr_path_stream << r.nr_txt;
            if (extractR) r_path_stream << r.r_txt;
            // printStatTable, :427-445: std::fixed << setprecision(5); kmers_in_seq is uint32 arithmetic and wraps for short records
            snprintf(line, sizeof line, "\t%u\t%.5f\t%.5f\t%u\t%u\t%u\t%.5f\t%u\t%.5f\t%.5f\n", r.median, r.mean, r.gc, r.length,
                     (uint32_t)(r.length - input.merLen + 1), r.invalid, r.percentInvalid, r.nonZero, r.percentNonZero, r.percentNonZeroCorrected);
            cvg_gc_stream << *r.name << line;
            if (r.mx_x < gcBins && r.mx_y < cvgBins) contamination_mx.data()[(size_t)r.mx_x * cvgBins + r.mx_y] += seqs[i].size();
        }
        katgpu_free_host(cvg);
        cvg = nullptr;
        katgpu_free_host(gct);
        gct = nullptr;
        lap(4);
        if (verbose) std::cerr << "done" << endl;
    }
    if (getenv("KATGPU_TIMING") && speak)
        fprintf(stderr, "katgpu_timing {\"phase\": \"sect_coverage\", \"read_s\": %.3f, \"join_s\": %.3f, \"device_call_s\": %.3f, \"records_s\": %.3f, \"text_s\": %.3f, \"gc_text_bytes\": %llu}\n",
                t_part[0], t_part[1], t_part[2], t_part[3], t_part[4], (unsigned long long)gc_text_bytes);
    cout << " done.";
    cout.flush();
}

int Sect::main(int argc, char* argv[]) {                                                        // src/sect.cc:604-741
    static const vector<OptSpec> spec = {
        {"output_prefix", 'o', true}, {"gc_bins", 'x', true}, {"cvg_bins", 'y', true}, {"cvg_logscale", 'l', false},
        {"threads", 't', true}, {"5ptrim", 0, true}, {"non_canonical", 'N', false}, {"mer_len", 'm', true}, {"hash_size", 'H', true},
        {"no_count_stats", 'n', false}, {"output_gc_stats", 'g', false}, {"extract_nr", 'E', false}, {"extract_r", 'F', false},
        {"min_repeat", 'M', true}, {"max_repeat", 'G', true}, {"dump_hash", 'd', false}, {"verbose", 'v', false}, {"help", 0, false}};
    ParsedArgs pa = parseArgs(argc, argv, spec);
    if (pa.has("help") || argc <= 1) {
        cout << "Usage: kat sect [options] <sequence_file> (<input>)+\n\nEstimates coverage levels across sequences in the provided input sequence file.\n" << endl;
        return 1;
    }
    vector<uint16_t> trim = parseTrimList(pa.get("5ptrim", "0"));
    PhaseTimer total("KAT SECT completed.\nTotal runtime: %.1fs\n\n");
    cout << "Running KAT in SECT mode" << endl << "------------------------" << endl << endl;
    string seq_file = pa.positional.empty() ? string() : pa.positional[0];                      // p.add("seq_file", 1); p.add("counts_files", -1)
    vector<string> counts_files(pa.positional.begin() + (pa.positional.empty() ? 0 : 1), pa.positional.end());
    Sect sect(counts_files, seq_file);
    sect.setOutputPrefix(pa.get("output_prefix", "kat-sect"));
    sect.setGcBins((uint16_t)std::stoul(pa.get("gc_bins", "1001")));
    sect.setCvgBins((uint16_t)std::stoul(pa.get("cvg_bins", "1001")));
    sect.setCvgLogscale(pa.has("cvg_logscale"));
    sect.setThreads((uint16_t)std::stoul(pa.get("threads", "1")));
    sect.setTrim(trim);
    sect.setCanonical(!pa.has("non_canonical"));
    sect.setMerLen((uint16_t)std::stoul(pa.get("mer_len", std::to_string(DEFAULT_MER_LEN))));
    sect.setHashSize(std::stoull(pa.get("hash_size", std::to_string(DEFAULT_HASH_SIZE))));
    sect.setNoCountStats(pa.has("no_count_stats"));
    sect.setOutputGCStats(pa.has("output_gc_stats"));
    sect.setExtractNR(pa.has("extract_nr"));
    sect.setExtractR(pa.has("extract_r"));
    sect.setMinRepeat((uint32_t)std::stoul(pa.get("min_repeat", "2")));
    sect.setMaxRepeat((uint32_t)std::stoul(pa.get("max_repeat", "0")));
    sect.setDumpHash(pa.has("dump_hash"));
    sect.setVerbose(pa.has("verbose"));
    sect.execute();         // the reference's main stops here: Sect::save() (the contamination matrix) is never called
    if (getenv("KATGPU_TESTING") && getenv("KATGPU_SECT_SAVE")) sect.save();     // test hook: exercises Sect::save() through the CLI
    return 0;
}

// ================================================================ Cold (src/cold.cc) ==============================
// Every record of the assembly against the reads hash and against the assembly's own hash: two
// katgpu_table_record_stats_host calls per batch, one -stats.tsv row per record.  --gpus N: the hashes lie on the ranks by owner, so
// the two calls are collective (katgpu_table_record_stats_gathered_host, no ranges): the counts are gathered on rank 0's device and
// reduced per record there; rank 0 writes the rows, the other ranks write nothing.

Cold::Cold(const vector<string>& reads_files, const string& asm_file) {                          // src/cold.cc:67-77
    reads.setMultipleInputs(reads_files);
    reads.index = 1;
    assembly.setSingleInput(asm_file);
    assembly.index = 1;                                                                         // sic: both inputs are "Input 1"
    outputPrefix = "kat-cold";
}

void Cold::execute() {                                                                           // src/cold.cc:80-122
    reads.validateInput();
    assembly.validateInput();
    ensureDirectoryExists(parentOfAbsolute(outputPrefix));
    // Cold never sets InputHandler::canonical (lib/include/kat/input_handler.hpp:48 defaults it to false): counted hashes
    // are non-canonical and probed as such; a loaded .jf brings its own flag.
    if (reads.mode == InputHandler::COUNT) reads.count(threads);
    else { reads.loadHeader(); reads.loadHash(); }
    if (assembly.mode == InputHandler::COUNT) assembly.count(threads);
    else { assembly.loadHeader(); assembly.loadHash(); }
    processSeqFile();
    if (dumpHashes()) {
        reads.dump(outputPrefix + "-reads_hash.jf" + std::to_string(reads.merLen), threads);
        assembly.dump(outputPrefix + "-asm_hash.jf" + std::to_string(assembly.merLen), threads);
    }
}

void Cold::processSeq(Row& r, const string& seq, const katgpu_record_stats& rd, const katgpu_record_stats& as) {   // src/cold.cc:303-408
    const uint16_t k = reads.merLen;
    const uint64_t seqLength = seq.size();
    const int64_t nbCounts = (int64_t)seqLength - k + 1;
    const uint64_t nbNonZero = rd.non_zero, nbInvalid = rd.invalid;
    r.median = 0; r.mean = 0.0; r.asmCn = 0;
    if (nbCounts > 0) {
        r.median = (uint32_t)(double)rd.median;
        r.mean = (double)rd.sum / (double)nbCounts;
        r.asmCn = (uint32_t)(double)as.median;
    }
    r.length = (uint32_t)seqLength;
    r.nonZero = (uint32_t)nbNonZero;
    r.percentNonZero = nbNonZero == 0 || nbCounts <= 0 ? 0.0 : ((double)nbNonZero / (double)nbCounts) * 100.0;
    r.invalid = (uint32_t)nbInvalid;
    r.percentInvalid = nbInvalid == 0 || nbCounts <= 0 ? 0.0 : ((double)nbInvalid / (double)nbCounts) * 100.0;
    const uint64_t notInvalid = (uint64_t)nbCounts - nbInvalid;
    r.percentNonZeroCorrected = nbNonZero == 0 || notInvalid <= 0 ? 0.0 : ((double)nbNonZero / (double)notInvalid) * 100.0;
    volatile double num = (double)rd.gc_bases, den = (double)(seqLength - rd.n_bases);
    r.gc = num / den;
}

void Cold::processSeqFile() {                                                                    // src/cold.cc:126-200
    PhaseTimer timer;
    cout << "Calculating kmer coverage across sequences ...";
    cout.flush();
    SeqRecordReader reader(assembly.pathString());
    if (verbose) std::cerr << endl;
    const bool dist = Engine::dist(), speak = !dist || Engine::speaker();
    std::ofstream cvg_gc_stream;
    if (speak) cvg_gc_stream.open((outputPrefix + "-stats.tsv").c_str());
    if (speak) cvg_gc_stream << "seq_name\tread_median_cvg\tread_mean_cvg\tasm_cn\tgc%\tseq_length\tkmers_in_seq\tinvalid_kmers\t%_invalid\tnon_zero_kmers\t%_non_zero\t%_non_zero_corrected" << endl;

    const size_t BATCH_BASES = (size_t)64 << 20;
    vector<string> names, seqs;
    vector<Row> rows;
    string joined;
    vector<katgpu_record_stats> rstats, astats;
    vector<uint64_t> offs, lens;
    while (!reader.atEnd()) {
        if (verbose) std::cerr << "Loading Batch of sequences... ";
        names.clear(); seqs.clear();
        size_t bases = 0;
        while (!reader.atEnd() && bases < BATCH_BASES) {
            names.emplace_back(); seqs.emplace_back();
            reader.readRecord(names.back(), seqs.back());
            bases += seqs.back().size() + 1;
        }
        const size_t n = names.size();
        if (verbose) std::cerr << "Loaded " << n << " records.  Processing batch... ";
        joined.clear(); joined.reserve(bases);
        offs.assign(n, 0); lens.assign(n, 0);
        for (size_t i = 0; i < n; i++) { offs[i] = joined.size(); lens[i] = seqs[i].size(); joined += seqs[i]; joined += '\n'; }
        rstats.resize(n); astats.resize(n);
        // the device reduces every record's counts: everything from the reads hash, the median (asm_cn) from the assembly's
        if (dist) {
            auto gathered = [&](InputHandler& in, vector<katgpu_record_stats>& st) {
                Engine::recordStatsGathered(in.hash, joined.data(), joined.size(), offs.data(), lens.data(), n, in.canonical, nullptr, 0,
                                            speak ? st.data() : nullptr, nullptr, nullptr);
            };
            gathered(reads, rstats);
            gathered(assembly, astats);
            if (!speak) continue;
        } else {
            Engine::check(katgpu_table_record_stats_host(reads.hash, joined.data(), joined.size(), offs.data(), lens.data(), n, reads.canonical ? 1 : 0, rstats.data()));
            Engine::check(katgpu_table_record_stats_host(assembly.hash, joined.data(), joined.size(), offs.data(), lens.data(), n, assembly.canonical ? 1 : 0, astats.data()));
        }

        rows.assign(n, Row());
        for (size_t i = 0; i < n; i++) processSeq(rows[i], seqs[i], rstats[i], astats[i]);
        char line[512];
        for (size_t i = 0; i < n; i++) {                                                        // printStatTable, src/cold.cc:254-271
            const Row& r = rows[i];
            snprintf(line, sizeof line, "\t%u\t%.5f\t%u\t%.5f\t%u\t%u\t%u\t%.5f\t%u\t%.5f\t%.5f\n", r.median, r.mean, r.asmCn, r.gc, r.length,
                     (uint32_t)(r.length - assembly.merLen + 1), r.invalid, r.percentInvalid, r.nonZero, r.percentNonZero, r.percentNonZeroCorrected);
            cvg_gc_stream << names[i] << line;
        }
        if (verbose) std::cerr << "done" << endl;
    }
    cout << " done.";
    cout.flush();
}

int Cold::main(int argc, char* argv[]) {                                                         // src/cold.cc:436-546
    static const vector<OptSpec> spec = {
        {"output_prefix", 'o', true}, {"gc_bins", 'x', true}, {"cvg_bins", 'y', true}, {"threads", 't', true}, {"5ptrim", 0, true},
        {"mer_len", 'm', true}, {"hash_size", 'H', true}, {"dump_hashes", 'd', false}, {"disable_hash_grow", 'g', false},
        {"output_type", 'p', true}, {"verbose", 'v', false}, {"help", 0, false}};
    ParsedArgs pa = parseArgs(argc, argv, spec);
    if (pa.has("help") || argc <= 1) {
        cout << "Usage: kat cold [options] <assembly> (<reads>)+\n\nCalculates median read k-mer coverage, assembly k-mer coverage and GC% across each sequence in the provided assembly.\n" << endl;
        return 1;
    }
    vector<uint16_t> trim = parseTrimList(pa.get("5ptrim", "0"));
    PhaseTimer total("KAT CoLD completed.\nTotal runtime: %.1fs\n\n");
    cout << "Running KAT in Cold mode" << endl << "------------------------" << endl << endl;
    string asm_file = pa.positional.empty() ? string() : pa.positional[0];                      // p.add("asm_file", 1); p.add("reads_files", -1)
    vector<string> reads_files(pa.positional.begin() + (pa.positional.empty() ? 0 : 1), pa.positional.end());
    Cold cold(reads_files, asm_file);
    cold.setOutputPrefix(pa.get("output_prefix", "kat-cold"));
    cold.setGcBins((uint16_t)std::stoul(pa.get("gc_bins", "1001")));
    cold.setCvgBins((uint16_t)std::stoul(pa.get("cvg_bins", "1001")));
    cold.setThreads((uint16_t)std::stoul(pa.get("threads", "1")));
    cold.setReadsTrim(trim);
    cold.setMerLen((uint8_t)std::stoul(pa.get("mer_len", std::to_string(DEFAULT_MER_LEN))));   // uint8_t setter, src/cold.hpp:160
    cold.setHashSize(std::stoull(pa.get("hash_size", std::to_string(DEFAULT_HASH_SIZE))));
    cold.setDumpHashes(pa.has("dump_hashes"));
    cold.setVerbose(pa.has("verbose"));
    // --disable_hash_grow is parsed and never applied in the reference's main (src/cold.cc:525-535)
    cold.execute();         // cold.plot() needs the Python plotting package: out of scope
    return 0;
}

}  // namespace kat
