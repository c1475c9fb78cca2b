// filter.cc -- `kat filter kmer` and `kat filter seq` (src/filter.cc, src/filter_kmer.cc, src/filter_sequence.cc).
//
// filter kmer: the reference walks every entry of the input hash with one region_iterator per thread and adds the chosen ones into one or
// two new hashes (FilterKmer::filterSlice); here that is one katgpu_table_filter call, which builds the new tables on the device and
// returns the three counters of FilterKmer::merge from the same pass.
// filter seq: the reference looks every window of every record up in the hash (FilterSeq::getProfile) and counts the hits; here a batch of
// records is joined into one base buffer and katgpu_table_seq_hits_host returns one hit count per record.  What stays on the host is
// what the reference does after the lookups: the keep decision, the subsampling draw and the output records, in input order.
// `katgpu filter seq --gpus N`: the hash lies on the ranks by owner and the per-record hits are summed over them on rank 0
// (katgpu_table_seq_hits_gathered_host), which alone decides and writes.  `filter kmer` stays on one GPU.
#include "kat_host.hpp"

#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <exception>
#include <fstream>
#include <iostream>
#include <random>

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

string pathExtension(const string& p) {          // boost::filesystem::path::extension
    const size_t slash = p.find_last_of('/');
    const string name = slash == string::npos ? p : p.substr(slash + 1);
    if (name == "." || name == "..") return "";
    const size_t dot = name.rfind('.');
    return dot == string::npos ? string() : name.substr(dot);
}

// seqan::SeqFileOut + writeRecord(file, meta, seq, qual) (deps/seqan-library-2.0.0/include/seqan/seq_io/fasta_fastq.h:455-505,
// stream/tokenization.h:464-482).  The format follows from the file name once a compression extension is taken off
// (stream/formatted_file.h:684-696); a name it cannot place is UnknownExtensionError -- a std::ios_base::failure, so `kat` exits 5 --
// thrown after the stream has been opened, which leaves an empty file behind.
class SeqWriter {
public:
    enum Format { FASTA, FASTQ, RAW, UNKNOWN };
    static Format formatOf(const string& path) {
        string base = path;
        for (const char* z : {".gz", ".bgzf", ".bz2"}) if (endsWithNoCase(base, z)) { base.resize(base.size() - strlen(z)); break; }
        if (base.size() != path.size()) return UNKNOWN;            // a compressed name is never followed by a sequence extension here (.in / .out / .R1 / .R2 come first)
        if (endsWithNoCase(base, ".fa") || endsWithNoCase(base, ".fasta")) return FASTA;
        if (endsWithNoCase(base, ".fq") || endsWithNoCase(base, ".fastq")) return FASTQ;
        if (endsWithNoCase(base, ".txt")) return RAW;
        return UNKNOWN;
    }
    // what opening `path` would throw, for a rank that opens nothing (--gpus: only rank 0 creates the files)
    static void checkName(const string& path) {
        if (formatOf(path) == UNKNOWN) throw std::runtime_error("Unknown file extension of " + path + ": iostream error");
    }
    explicit SeqWriter(const string& path) : os(path.c_str(), std::ios::binary | std::ios::trunc), fmt(formatOf(path)) {
        if (!os) throw std::runtime_error("Could not open file " + path + ": iostream error");
        if (fmt == UNKNOWN) { os.close(); throw std::runtime_error("Unknown file extension of " + path + ": iostream error"); }
    }
    void write(const string& name, const string& seq, const string& qual) {
        if (fmt == FASTA) { buf += '>'; buf += name; buf += '\n'; wrapped(seq, 70); }
        else if (fmt == FASTQ) { buf += '@'; buf += name; buf += '\n'; wrapped(seq, 0); buf += "+\n"; wrapped(qual, 0); }
        else { buf += seq; buf += '\n'; }
        if (buf.size() >= ((size_t)4 << 20)) flush();
    }
    void flush() { os.write(buf.data(), (std::streamsize)buf.size()); buf.clear(); }
    ~SeqWriter() { flush(); }
private:
    void wrapped(const string& s, size_t line) {            // writeWrappedString: at least one line, even for an empty string
        if (!line) line = s.size() ? s.size() : 1;
        size_t at = 0;
        do {
            const size_t n = std::min(s.size() - at, line);
            buf.append(s, at, n);
            buf += '\n';
            at += n;
        } while (at < s.size());
    }
    std::ofstream os;
    string buf;
    Format fmt = UNKNOWN;
};

uint64_t nbKmers(size_t len, uint16_t k) { return len >= k ? (uint64_t)(len - k + 1) : 0; }   // getProfile's nbCounts, 0 when <= 0
}  // namespace

// ---------------------------------------------------------------------------------------------- filter kmer ----

FilterKmer::FilterKmer(const vector<string>& inputs) { input.setMultipleInputs(inputs); }       // src/filter_kmer.cc:92-117

void FilterKmer::execute() {                                                                    // src/filter_kmer.cc:119-190
    if (high_count < low_count) throw FilterKmerException("High kmer count value must be >= to low kmer count value");
    if (high_gc < low_gc) throw FilterKmerException("High GC count value must be >= to low GC count value");
    input.validateInput();
    ensureDirectoryExists(parentOfAbsolute(output_prefix));
    if (input.mode == InputHandler::COUNT) input.count(threads);
    else { input.loadHeader(); input.loadHash(); }
    if (verbose) {
        uint64_t capacity = 0;
        Engine::check(katgpu_table_stats(input.hash, nullptr, nullptr, &capacity));
        std::cerr << "Attempting to create output hash with the following settings: " << endl
                  << " mer len           - " << input.merLen << endl
                  << " hash size         = " << capacity << endl << endl;
    }
    filter();
    merge();
    const string k = std::to_string(input.merLen);
    dump(output_prefix + "-in.jf" + k, in_hash);
    if (separate) dump(output_prefix + "-out.jf" + k, out_hash);
    katgpu_table_free(in_hash); in_hash = nullptr;
    katgpu_table_free(out_hash); out_hash = nullptr;
}

void FilterKmer::filter() {                                                                     // src/filter_kmer.cc:232-249
    PhaseTimer timer;
    cout << "Filtering kmers ...";
    cout.flush();
    Engine::check(katgpu_table_filter(input.hash, low_count, high_count, low_gc, high_gc, invert ? 1 : 0, separate ? 1 : 0, &in_hash,
                                      separate ? &out_hash : nullptr, counters));
    cout << " done.";
    cout.flush();
}

void FilterKmer::merge() {                                                                      // src/filter_kmer.cc:212-230
    auto line = [](uint64_t d, uint64_t t) { return std::to_string(d) + " distinct; " + std::to_string(t) + " total."; };
    cout << "K-mers in input   : " << line(counters[0], counters[1]) << endl
         << "K-mers to keep    : " << line(counters[2], counters[3]) << endl;
    if (separate) cout << "K-mers to discard : " << line(counters[4], counters[5]) << endl;
    cout << endl;
}

void FilterKmer::dump(const string& path, katgpu_table* hash) {                                 // src/filter_kmer.cc:192-210
    struct stat st;
    if (lstat(path.c_str(), &st) == 0) unlink(path.c_str());
    PhaseTimer timer;
    cout << "Dumping hash to " << path << " ...";
    cout.flush();
    if (katgpu_jf_dump(hash, path.c_str())) throw JellyfishException(*katgpu_jf_last_error() ? katgpu_jf_last_error() : katgpu_last_error(Engine::ctx()));
    cout << " done.";
    cout.flush();
}

int FilterKmer::main(int argc, char* argv[]) {                                                  // src/filter_kmer.cc:310-415
    static const vector<OptSpec> spec = {
        {"output_prefix", 'o', true}, {"threads", 't', true}, {"low_count", 'c', true}, {"high_count", 'd', true}, {"low_gc", 'g', true},
        {"high_gc", 'h', true}, {"invert", 'i', false}, {"separate", 's', false}, {"non_canonical", 'N', false}, {"mer_len", 'm', true},
        {"hash_size", 'H', true}, {"verbose", 'v', false}, {"help", 0, false}};
    ParsedArgs pa = parseArgs(argc, argv, spec);
    if (pa.has("help") || argc <= 1) {
        cout << "Usage: kat filter kmer [options] (<input>)+\n\nFilter kmers from a k-mer hash or from k-mers counted in sequence files.\n" << endl;
        return 1;
    }
    PhaseTimer total("KAT filter kmer completed.\nTotal runtime: %.1fs\n\n");
    cout << "Running KAT in filter kmer mode" << endl << "-------------------------------" << endl << endl;
    FilterKmer filter(pa.positional);
    filter.setLow_count(std::stoull(pa.get("low_count", "1")));
    filter.setHigh_count(std::stoull(pa.get("high_count", "10000")));
    filter.setLow_gc((uint16_t)std::stoul(pa.get("low_gc", "1")));
    filter.setHigh_gc((uint16_t)std::stoul(pa.get("high_gc", "100")));
    filter.setOutput_prefix(pa.get("output_prefix", "kat.filter.kmer"));
    filter.setThreads((uint16_t)std::stoul(pa.get("threads", "1")));
    filter.setCanonical(!pa.has("non_canonical"));
    filter.setInvert(pa.has("invert"));
    filter.setSeparate(pa.has("separate"));
    filter.setMerLen((uint16_t)std::stoul(pa.get("mer_len", std::to_string(DEFAULT_MER_LEN))));
    filter.setHashSize(std::stoull(pa.get("hash_size", std::to_string(DEFAULT_HASH_SIZE))));
    filter.setVerbose(pa.has("verbose"));
    filter.execute();
    return 0;
}

// ----------------------------------------------------------------------------------------------- filter seq ----

FilterSeq::FilterSeq(const string& s1, const string& s2, const vector<string>& inputs) : seq_file_1(s1), seq_file_2(s2) {   // :48-80
    input.setMultipleInputs(inputs);
}

FilterSeq::~FilterSeq() = default;

void FilterSeq::execute() {                                                                     // src/filter_sequence.cc:82-150
    struct stat st;
    if (lstat(seq_file_1.c_str(), &st) != 0 || stat(seq_file_1.c_str(), &st) != 0)
        throw FilterSeqException("Could not find input file at: " + seq_file_1 + "; please check the path and try again.");
    if (isPaired() && (lstat(seq_file_2.c_str(), &st) != 0 || stat(seq_file_2.c_str(), &st) != 0))
        throw FilterSeqException("Could not find sequence file at: " + seq_file_2 + "; please check the path and try again.");
    input.validateInput();
    ensureDirectoryExists(parentOfAbsolute(output_prefix));
    if (input.mode == InputHandler::COUNT) input.count(threads);
    else { input.loadHeader(); input.loadHash(); }
    processSeqFile();
    cout << "Found " << keepers << " / " << total << " to keep" << endl << endl;
}

void FilterSeq::processSeqFile() {                                                              // src/filter_sequence.cc:152-281, 283-353
    PhaseTimer timer;
    cout << "Filtering sequences ..." << endl;
    SeqRecordReader reader(seq_file_1);
    std::unique_ptr<SeqRecordReader> reader2;
    if (isPaired()) reader2.reset(new SeqRecordReader(seq_file_2));
    // --gpus N: the hash lies on the ranks by owner, every rank reads the sequence file(s) and cuts the same batches, and the hits reach
    // rank 0 through one collective per batch (katgpu_table_seq_hits_gathered_host).  Rank 0 alone opens the outputs, draws the random
    // numbers, decides and writes; the other ranks create nothing -- but look at the output names as rank 0 does when it opens them, and one
    // all-reduce in front of the batches tells every rank whether any was refused: all ranks end there with the plain run's error.
    const bool dist = Engine::dist(), speak = !dist || Engine::speaker();
    std::ofstream stats;
    if (doStats && speak) {
        stats.open((output_prefix + ".stats").c_str());
        stats << "index\tnb_bases\tnb_kmers\tnb_hits\tratio" << endl;
    }
    const string ext = pathExtension(seq_file_1);
    const string r1 = isPaired() ? ".R1" : "";
    std::unique_ptr<SeqWriter> inW, outW, inW2, outW2;
    auto open = [&](std::unique_ptr<SeqWriter>& w, const string& path) { if (speak) w.reset(new SeqWriter(path)); else SeqWriter::checkName(path); };
    std::exception_ptr refused;
    try {
        open(inW, output_prefix + ".in" + r1 + ext);
        if (separate) open(outW, output_prefix + ".out" + r1 + ext);
        if (isPaired()) {
            open(inW2, output_prefix + ".in.R2" + ext);
            if (separate) open(outW2, output_prefix + ".out.R2" + ext);
        }
    } catch (...) { refused = std::current_exception(); }
    if (dist) {                                              // all go on, or none does: rank 0 has left what the plain run leaves by the time the others end
        uint64_t n_refused = refused ? 1 : 0;
        Engine::allreduce(&n_refused, 1);
        if (n_refused && !refused) refused = std::make_exception_ptr(std::runtime_error("Could not open the output files of rank 0: iostream error"));
    }
    if (refused) std::rethrow_exception(refused);
    std::random_device rd;
    std::mt19937 gen(speak ? rd() : 0u);
    std::uniform_real_distribution<> urd;
    const uint16_t k = input.merLen;
    const int per = isPaired() ? 2 : 1;                      // device records per entry: R1 (and R2)

    // Bounded batches: the reference handles one record at a time; here up to BATCH_ENTRIES records or pairs (or BATCH_BASES bases) go
    // to the device together, so host memory stays the same whatever the input's size.
    const size_t BATCH_ENTRIES = (size_t)1 << 20, BATCH_BASES = (size_t)256 << 20;
    vector<string> names, seqs, quals;
    string joined;
    vector<uint64_t> starts, lens, hits;
    vector<double> vals;
    uint64_t index = 0;
    while (!reader.atEnd()) {
        size_t n = 0, bases = 0;
        while (!reader.atEnd() && n < BATCH_ENTRIES && bases < BATCH_BASES) {
            if (names.size() < (n + 1) * per) { names.resize((n + 1) * per); seqs.resize((n + 1) * per); quals.resize((n + 1) * per); }
            reader.readRecord(names[n * per], seqs[n * per], quals[n * per]);
            bases += seqs[n * per].size();
            if (isPaired()) { reader2->readRecord(names[n * per + 1], seqs[n * per + 1], quals[n * per + 1]); bases += seqs[n * per + 1].size(); }
            ++n;
        }
        const size_t nr = n * per;
        joined.clear(); joined.reserve(bases);
        starts.resize(nr); lens.resize(nr); hits.assign(nr, 0);
        for (size_t i = 0; i < nr; i++) { starts[i] = joined.size(); lens[i] = seqs[i].size(); joined += seqs[i]; }
        if (dist) Engine::seqHitsGathered(input.hash, joined.data(), joined.size(), starts.data(), lens.data(), nr, input.canonical, speak ? hits.data() : nullptr);
        else Engine::check(katgpu_table_seq_hits_host(input.hash, joined.data(), joined.size(), starts.data(), lens.data(), nr, input.canonical ? 1 : 0, hits.data()));
        for (size_t e = 0; speak && e < n; e++) {
            const double val = urd(gen);                                                       // drawn for every entry, in input order
            uint64_t nbFound = 0, nb = 0, len = 0;
            for (int q = 0; q < per; q++) { nbFound += hits[e * per + q]; nb += nbKmers(seqs[e * per + q].size(), k); len += seqs[e * per + q].size(); }
            volatile double num = (double)nbFound, den = (double)nb;                           // run-time division: 0/0 is the x86 default NaN ("-nan")
            const double ratio = num / den;
            bool keep = true;
            if ((ratio >= threshold && !invert) || (invert && ratio < threshold)) {
                if (frequency > 0.0 && frequency < val) keep = false;
                else {
                    keepers++;
                    inW->write(names[e * per], seqs[e * per], quals[e * per]);
                    if (isPaired()) inW2->write(names[e * per + 1], seqs[e * per + 1], quals[e * per + 1]);
                }
            } else keep = false;
            if (separate && !keep) {
                outW->write(names[e * per], seqs[e * per], quals[e * per]);
                if (isPaired()) outW2->write(names[e * per + 1], seqs[e * per + 1], quals[e * per + 1]);
            }
            if (doStats) stats << index << "\t" << len << "\t" << nb << "\t" << nbFound << "\t" << ratio << "\n";
            total++;
            index++;
            if (index % 100000 == 0) cout << "Processed " << index << (isPaired() ? " pairs" : " entries") << endl;
        }
    }
    if (isPaired() && !reader2->atEnd()) throw FilterSeqException("Second sequence file appears to be longer than the first.");
    inW.reset(); outW.reset(); inW2.reset(); outW2.reset();
    if (stats.is_open()) stats.close();
    cout << "Finished filtering.";
    cout.flush();
}

int FilterSeq::main(int argc, char* argv[]) {                                                   // src/filter_sequence.cc:355-480
    static const vector<OptSpec> spec = {
        {"output_prefix", 'o', true}, {"threads", 't', true}, {"threshold", 'T', true}, {"invert", 'i', false}, {"separate", 's', false},
        {"seq", 0, true}, {"seq2", 0, true}, {"frequency", 'f', true}, {"stats", 0, false}, {"non_canonical", 'N', false},
        {"mer_len", 'm', true}, {"hash_size", 'H', true}, {"verbose", 'v', false}, {"help", 0, false}};
    ParsedArgs pa = parseArgs(argc, argv, spec);
    if (pa.has("help") || argc <= 1) {
        cout << "Usage: kat filter seq [options] --seq <seq_file> [--seq2 <seq_file2>] (<input>)+\n\nFilter sequences by the k-mers of a hash.\n" << endl;
        return 1;
    }
    const string seq1 = pa.get("seq", ""), seq2 = pa.get("seq2", "");
    if (seq1.empty()) throw FilterSeqException("You must specify at least one sequence file to filter");
    PhaseTimer total("KAT filter seq completed.\nTotal runtime: %.1fs\n\n");
    cout << "Running KAT in filter sequence mode" << endl << "-----------------------------------" << endl << endl;
    FilterSeq filter(seq1, seq2, pa.positional);
    filter.setThreshold(std::stod(pa.get("threshold", "0.1")));
    filter.setOutput_prefix(pa.get("output_prefix", "kat.filter.kmer"));                          // (sic: the reference's default)
    filter.setThreads((uint16_t)std::stoul(pa.get("threads", "1")));
    filter.setCanonical(!pa.has("non_canonical"));
    filter.setInvert(pa.has("invert"));
    filter.setSeparate(pa.has("separate"));
    filter.setFrequency(std::stod(pa.get("frequency", "0.0")));
    filter.setDoStats(pa.has("stats"));
    filter.setMerLen((uint16_t)std::stoul(pa.get("mer_len", std::to_string(DEFAULT_MER_LEN))));
    filter.setHashSize(std::stoull(pa.get("hash_size", std::to_string(DEFAULT_HASH_SIZE))));
    filter.setVerbose(pa.has("verbose"));
    filter.execute();
    return 0;
}

// -------------------------------------------------------------------------------------------------- filter ----

int Filter::main(int argc, char* argv[]) {                                                      // src/filter.cc:60-131
    // the mode is the first positional argument; -v / --help alone print the usage (exit 1, as every mode's help here)
    int at = 1;
    while (at < argc && (!strcmp(argv[at], "-v") || !strcmp(argv[at], "--verbose") || !strcmp(argv[at], "--help"))) ++at;
    if (at >= argc) {
        cout << "Usage: kat filter <mode>\n\nFilter a k-mer hash or a sequence file.  Modes: kmer, seq\n" << endl;
        return 1;
    }
    const string mode = argv[at];
    string upper = mode;
    for (auto& ch : upper) ch = (char)toupper((unsigned char)ch);
    // an unrecognised mode is a KatFilterException (exit 4) in the reference; this build reports it as a command-line error, exit 1
    if (upper == "KMER") return FilterKmer::main(argc - at, argv + at);
    if (upper == "SEQ") return FilterSeq::main(argc - at, argv + at);
    throw OptionError("Could not recognise mode string: " + mode + " (filter modes: kmer, seq)");
}

}  // namespace kat
